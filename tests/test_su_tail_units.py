"""Tail units of the shift-uniform kernel (csrc/tdr_score_su.hip; tdr_config_tuning "su_tail_groups" = K, "su_tail_parts" = Q):
the last K ring groups of the grid go as Q rows of 8 / Q sectors each, so that the workgroups dispatched last are short.  The
sums are exact integers and a row is only another partition of a window: the raw weights are the same BITS for every K, Q,
and the workspace tdr_score_workspace_floats names holds the rows of the largest split.  Run with `pytest -m gpu`.

The far-path case scores the scene on a map sixteen tiles wide (128 x 2048): on the 128 x 128 map itself the known mask of
the WHOLE map fits a wave's quarter of the staging area, so no wave could ever leave the staged path there."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TOTAL = 1_000_000
NCLS = 3
SPLITS = ((0, 1), (1, 2), (2, 4), (1 << 20, 8))   # (K, Q); the last: every group, eight parts
SHAPES = {  # nb, nr, su_group, span of the dense share (cells), map tiles side by side
    "8-ring groups": (32, 24, 8, 8.0, 1),
    "ragged 4-ring groups, sectors of 5": (40, 22, 4, 8.0, 1),
    "a wave on the far path": (32, 24, 8, 1e9, 16),
}


@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pkg, HipKernels()


def _scene(nb, nr, tiles):
    """Three classes on a 128 x 128 map (`tiles` of it side by side) that is known everywhere but in one hole; 512 particles
    of two heading bins within a few cells of (64, 64) — the windows of the sectors that look towards the hole reach it, those
    of the others see known cells only — and 16 far from them and from each other: with one tile, spread over the map at
    headings of their own (the ray-mapped kernel's share); with several, one per tile at ONE third heading — a wave of the
    shift-uniform kernel whose windows no staged box can hold."""
    from top_down_renderer_amd import synth
    cfg = synth.Config("tail", 4000, NCLS, nb, nr, 128, 528, seed=6100 + nb)
    sc = synth.make_scene(cfg)
    maps = sc.class_maps.copy()
    mask = np.zeros((128, 128), np.uint8)
    mask[78:84, 78:84] = 1
    maps[:, mask == 1] = 0
    maps, mask = np.tile(maps, (1, 1, tiles)), np.tile(mask, (1, tiles))
    rng = np.random.default_rng(nb * 100 + nr)
    st = np.zeros(528, synth.STATE_DTYPE)
    st["scale"] = 1.0
    st["have_init"] = 1
    st["init_x_px"][:512] = rng.normal(64.0, 1.0, 512).clip(60.5, 67.5)
    st["init_y_px"][:512] = rng.normal(64.0, 1.0, 512).clip(60.5, 67.5)
    st["theta"][:200] = 2 * np.pi * 3 / nb            # heading bin 3: 200 particles, 56 padding slots
    st["theta"][200:512] = 2 * np.pi * 5 / nb         # heading bin 5: 312 particles, five waves
    if tiles == 1:
        gx, gy = np.meshgrid([16.0, 48.0, 80.0, 112.0], [16.0, 48.0, 80.0, 112.0])
        st["init_x_px"][512:] = gx.ravel() + 0.25
        st["init_y_px"][512:] = gy.ravel() + 0.25
        st["theta"][512:] = rng.uniform(-np.pi, np.pi, 16)
    else:
        st["init_x_px"][512:] = 64.0 + 128.0 * np.arange(16)
        st["init_y_px"][512:] = np.linspace(20.0, 108.0, 16)
        st["theta"][512:] = 2 * np.pi * 17 / nb
    return sc, maps.astype(np.float32), mask, st


def _knobs(k, **kw):
    for name, v in kw.items():
        assert k.lib.tdr_config_tuning(name.encode(), int(v)) >= 0, name


@pytest.fixture(scope="module")
def saved_knobs(tdr):
    _, k = tdr
    names = ("su_tail_groups", "su_tail_parts", "su_group")
    before = {n: int(k.lib.tdr_config_tuning(n.encode(), -1)) for n in names}
    mode = k.lib.tdr_config_shift_uniform(-1)

    def restore():
        _knobs(k, **before)
        k.lib.tdr_config_shift_uniform(mode)
        k.lib.tdr_config_shift_uniform_span(-2.0)
        k.lib.tdr_profile_enable(0)
    return restore


def _setup(tdr, oracle, nb, nr, tiles):
    import torch
    pkg, k = tdr
    sc, maps, mask, st = _scene(nb, nr, tiles)
    cfg = sc.cfg
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, mask, kernels=k)
    assert m.dev.desc.cwords > 0
    m.samplePtsPolar((nb, nr), cfg.ang_res)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, NCLS, nb, nr)
    f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False, locality_every=1)
    f.set_states(st)
    perm = k.zeros((f.cap_local,), torch.int32)
    k.locality_order(f.st, len(st), m.rows, m.cols, perm)
    return cfg, m, m.scan_handle(scan), f, perm, len(st)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tail_units_leave_every_bit_of_the_weights(tdr, oracle, saved_knobs, shape):
    pkg, k = tdr
    nb, nr, su_group, span, tiles = SHAPES[shape]
    cfg, m, pk, f, perm, n = _setup(tdr, oracle, nb, nr, tiles)

    def run():
        f.raw_w.fill_(-7.0)
        k.score(m.dev, pk, float(cfg.res), f.fp_c, f.st, n, f.raw_w, perm=perm, uniform_scale=f._uniform_scale, n_total=N_TOTAL)
        k.synchronize()
        return f.raw_w[:n].cpu().numpy()

    got = {}
    try:
        k.lib.tdr_config_shift_uniform_span(span)
        k.lib.tdr_config_shift_uniform(0)
        raw_float = run()
        k.lib.tdr_config_shift_uniform(2)   # small shapes take the integer form too
        _knobs(k, su_group=su_group)
        for kq in SPLITS:
            _knobs(k, su_tail_groups=kq[0], su_tail_parts=kq[1])
            if kq == (0, 1):   # what the scene promises, from the kernels' own counters
                k.lib.tdr_profile_enable(2)
            launches = int(k.lib.tdr_shift_uniform_launches())
            got[kq] = run()
            assert int(k.lib.tdr_shift_uniform_launches()) == launches + 1
            if kq == (0, 1):
                v = (C.c_int64 * 16)()
                assert k.lib.tdr_profile_variants(v) == 0
                d_ms, s_ms, s_n = C.c_double(0), C.c_double(0), C.c_int64(0)
                assert k.lib.tdr_profile_shares(C.byref(d_ms), C.byref(s_ms), C.byref(s_n)) == 0
                k.lib.tdr_profile_enable(0)
                all_known, others, far = v[0] + v[3], v[1] + v[2] + v[4] + v[5], v[6]
                if tiles == 1:
                    assert all_known > 0 and others > 0, list(v)[:7]    # all-known and not-all-known sectors both occur
                    assert 0 < s_n.value < n                            # both kernels ran
                else:
                    assert far > 0, list(v)[:7]                         # a wave took the far path
    finally:
        saved_knobs()
    ref = got[(0, 1)]
    assert not (ref == -7.0).any() and np.isnan(ref).sum() < n
    for kq in SPLITS[1:]:
        assert np.array_equal(np.isnan(got[kq]), np.isnan(ref)), kq
        assert np.array_equal(got[kq], ref, equal_nan=True), kq
    # the float form, to its rounding (tests/test_ray.py, tests/test_shift_uniform.py: 3e-6)
    assert np.array_equal(np.isnan(raw_float), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(raw_float[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    assert err.max(initial=0.0) <= 3e-6, err.max()


def test_the_workspace_holds_the_rows_of_the_largest_split(tdr, oracle, saved_knobs):
    """K = every group, Q = 8 — the most the knobs accept: eight rows per ring group.  The call gets a workspace of exactly
    tdr_score_workspace_floats(...) floats with canary words behind it."""
    import torch
    from top_down_renderer_amd.kernels import _ptr
    from top_down_renderer_amd._lib import check
    pkg, k = tdr
    nb, nr, su_group, span, tiles = SHAPES["ragged 4-ring groups, sectors of 5"]
    cfg, m, pk, f, perm, n = _setup(tdr, oracle, nb, nr, tiles)
    CANARY, WORDS = 0x5CA1AB1E, 4096
    try:
        k.lib.tdr_config_shift_uniform_span(span)
        k.lib.tdr_config_shift_uniform(2)
        _knobs(k, su_group=su_group, su_tail_groups=0, su_tail_parts=1)
        plain = int(k.lib.tdr_score_workspace_floats(NCLS, nb, nr, n, N_TOTAL))
        _knobs(k, su_tail_groups=1 << 20, su_tail_parts=8)
        assert k.lib.tdr_config_tuning(b"su_tail_groups", -1) == 1 << 20 and k.lib.tdr_config_tuning(b"su_tail_parts", -1) == 8
        need = int(k.lib.tdr_score_workspace_floats(NCLS, nb, nr, n, N_TOTAL))
        assert need > plain   # 48 rows of partial sums where 6 were
        buf = torch.full((need + WORDS,), CANARY, dtype=torch.int32, device=k.device)
        launches = int(k.lib.tdr_shift_uniform_launches())
        f.raw_w.fill_(-7.0)
        check(k.lib.tdr_k_score_polar_ctx(C.byref(m.dev.desc), _ptr(m.dev.tab), _ptr(pk), nb, nr, C.c_float(cfg.res),
                                          C.byref(f.fp_c), _ptr(f.st), f.st.shape[1], n, N_TOTAL, _ptr(perm),
                                          C.c_float(f._uniform_scale), 0, _ptr(f.raw_w), _ptr(buf), C.c_void_p(0), k.stream()))
        k.synchronize()
        assert int(k.lib.tdr_shift_uniform_launches()) == launches + 1
        assert not (f.raw_w[:n] == -7.0).any().item()
        assert (buf[need:] == CANARY).all().item()
    finally:
        saved_knobs()
