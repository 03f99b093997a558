"""The ray-mapped kernel's compact bin lists and its gate count (csrc/tdr_score_ray.hip, score_prep_kernel in
csrc/tdr_score_su.hip): with a caller's context that holds the table's factors and a direction count that is a multiple of
16, a wave walks lists of a sector's non-empty bins, and the empty bins only until the particle's known count is decided.
The weights must be the bits of the shift-uniform kernel and of the ray-mapped kernel in its ray order, the NaN pattern must
be the gate's at known counts just below, at and just above half the samples, and the counters of tdr_profile_ray_gate must
see every way a particle's count can end.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TOTAL = 1_000_000
ALL_RAY = 1e-6
NCLS = 6
SHAPES = [(16, 16), (48, 20), (64, 24), (256, 64)]          # a single unit; a ragged last ring block; ...; four segments
SCANS = ["empty", "full", "alternating", "listed", "frac20", "frac50", "frac80"]


@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pkg, HipKernels()


@pytest.fixture()
def restore(tdr):
    lib = tdr[1].lib
    before = lib.tdr_config_shift_uniform(-1)
    yield lib
    lib.tdr_config_shift_uniform(before)
    lib.tdr_config_shift_uniform_span(-2.0)
    lib.tdr_config_ray_split(0)
    lib.tdr_config_tuning(b"ray_patch", 1)
    lib.tdr_profile_enable(0)


def make_scan(kind, nb, nr, seed=0):
    """(NCLS, nb * nr) counts, bin (row i, ring j) at j * nb + i."""
    rng = np.random.default_rng(1000 + seed)
    i, j = np.meshgrid(np.arange(nb), np.arange(nr), indexing="xy")       # [j, i]
    cls = np.full((nr, nb), -1)
    cnt = np.zeros((nr, nb), np.float32)
    scan = np.zeros((NCLS, nr, nb), np.float32)
    if kind == "full":
        cls[:], cnt[:] = 2, 3
    elif kind == "alternating":       # class runs of unequal length inside a unit, some classes absent, some bins empty
        cls = (i * i + 3 * j) % 7
        cls[cls == 6] = -1
        cls[(cls == 4) & (i % 16 < 11)] = 1
        cnt[:] = 1 + (i + j) % 5
    elif kind == "listed":            # bins with two classes and counts >= 4096 (the list), among single-class ones
        cls = rng.integers(-1, NCLS, (nr, nb))
        cnt = rng.integers(1, 9, (nr, nb)).astype(np.float32)
        big = rng.random((nr, nb)) < 0.05
        cnt[big] = rng.integers(4096, 20000, int(big.sum()))
    elif kind.startswith("frac"):
        cls = np.where(rng.random((nr, nb)) < int(kind[4:]) / 100.0, rng.integers(0, NCLS, (nr, nb)), -1)
        cnt = rng.integers(1, 9, (nr, nb)).astype(np.float32)
    for c in range(NCLS):
        scan[c][cls == c] = cnt[cls == c]
    if kind == "listed":
        two = (rng.random((nr, nb)) < 0.07) & (cls >= 0)
        scan[(cls[two] + 1) % NCLS, j[two], i[two]] = 5
        assert ((scan != 0).sum(0) == 2).any() and (scan >= 4096).any()
    return np.ascontiguousarray(scan.reshape(NCLS, nr * nb))


class Rig:
    """One map, table and filter of a shape; run(...) scores the filter's particles one way."""

    def __init__(self, tdr, nb, nr, states, maps, mask):
        import torch
        pkg, k = tdr
        self.k, self.nb, self.nr, self.n = k, nb, nr, len(states)
        self.ang_res = np.float32(2 * np.pi / nb)
        self.m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, mask, kernels=k)
        self.m.samplePtsPolar((nb, nr), self.ang_res)
        self.f = pkg.ParticleFilter(self.n, self.m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False,
                                    locality_every=1)
        self.f.set_states(states)
        self.ctx = k.score_ctx_create()
        self.torch = torch

    def run(self, scan, span, split=0, patch=1, ctx=True):
        k, f, lib = self.k, self.f, self.k.lib
        lib.tdr_config_shift_uniform(2)
        lib.tdr_config_shift_uniform_span(span)
        lib.tdr_config_ray_split(split)
        lib.tdr_config_tuning(b"ray_patch", patch)
        f.raw_w.fill_(-7.0)
        k.score(self.m.dev, self.m.scan_handle(scan), 1.0, f.fp_c, f.st, self.n, f.raw_w, uniform_scale=f._uniform_scale,
                n_total=N_TOTAL, ctx=self.ctx if ctx else None)
        k.synchronize()
        out = f.raw_w[: self.n].cpu().numpy()
        assert not (out == -7.0).any()
        return out


def gate_counters(lib):
    out = (C.c_int64 * 4)()
    assert lib.tdr_profile_ray_gate(out) == 0
    return [int(v) for v in out]


_scene_cache = {}


def scene_rig(tdr, nb, nr):
    if (nb, nr) not in _scene_cache:
        from top_down_renderer_amd import synth
        sc = synth.make_scene(synth.Config("compact", 2000, NCLS, nb, nr, 260, 128, seed=6100 + nr))
        st = sc.states.copy()
        st["init_x_px"][::9] = np.random.default_rng(nr).uniform(-60, 320, len(st[::9])).astype(np.float32)   # borders, outside
        _scene_cache[(nb, nr)] = (Rig(tdr, nb, nr, st, sc.class_maps, sc.class_mask), st, sc)
    return _scene_cache[(nb, nr)]


@pytest.mark.parametrize("kind", SCANS)
@pytest.mark.parametrize("nb,nr", SHAPES)
def test_three_ways_one_set_of_bits(tdr, oracle, restore, nb, nr, kind):
    """Compact lists (context with factors), the shift-uniform kernel and the ray order give the same raw weights, which are
    the oracle's to 1e-5 with its NaN pattern.  An all-non-empty scan walks no B block at all."""
    rig, st, sc = scene_rig(tdr, nb, nr)
    scan = make_scan(kind, nb, nr, seed=nb + nr)
    restore.tdr_profile_enable(2)
    gate_counters(restore)
    new = rig.run(scan, ALL_RAY)
    ctr = gate_counters(restore)
    restore.tdr_profile_enable(0)
    assert sum(ctr[:3]) == rig.n, ctr                   # every particle ended one of the three ways: the new path ran
    if kind == "full":
        assert ctr[3] == 0 and ctr[1] == 0, ctr         # (nothing to walk, whether the particle's waves share the count or not)
    assert np.array_equal(new, rig.run(scan, 0.0), equal_nan=True), "shift-uniform kernel"
    assert np.array_equal(new, rig.run(scan, ALL_RAY, patch=0), equal_nan=True), "ray order"
    ref = oracle.compute_weights(oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0), oracle.polar_table(nb, nr, rig.ang_res),
                                 nb, nr, scan, 1.0, oracle.make_params(NCLS), st.copy())
    assert np.array_equal(np.isnan(new), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(new[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    assert err.max(initial=0.0) <= 1e-5, err.max()


def gate_map(kind, size=240):
    """Class distances of a synthetic scene under a mask whose unknown cells are a half-plane / every third row and column."""
    from top_down_renderer_amd import synth
    sc = synth.make_scene(synth.Config("gate", 2000, NCLS, 64, 24, size, 8, seed=6200))
    mask = np.zeros((size, size), np.uint8)
    if kind == "half":    # a slanted edge: as a particle moves across it the samples change sides one at a time
        yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
        mask[xx + 0.31 * yy < 150] = 1
    else:
        mask[::3, :] = 1
        mask[:, ::3] = 1
    maps = sc.class_maps.copy()
    maps[:, mask == 1] = 0
    return maps, mask


def line_particles(oracle, om, tab, P, n_cand, targets, n_keep):
    """Candidates on a line across the half-plane's edge (start and step found on the CPU so that known counts of P/2 - 1,
    P/2 and P/2 + 1 occur); every candidate's TRUE known count (the oracle's mask); keep the targets and an even sample."""
    from oracle.c_oracle import STATE_DTYPE
    t = np.linspace(0.0, 1.0, n_cand)
    x = (100.3 + 41.0 * t).astype(np.float32)
    y = (96.0 + 48.0 * t).astype(np.float32)
    known = np.array([P - int(oracle.local_map_polar(om, tab, float(x[q]), float(y[q]), 1.0, 1.0)[1].sum()) for q in range(n_cand)])
    pick = []
    for want in targets:
        hit = np.flatnonzero(2 * known == want)
        assert len(hit), f"no candidate on the line has 2 * known = {want} (P = {P}): change the line"
        pick += [int(hit[0]), int(hit[-1])]
    pick = sorted(set(pick) | set(np.linspace(0, n_cand - 1, n_keep - len(set(pick))).astype(int).tolist()))
    st = np.zeros(len(pick), STATE_DTYPE)
    st["init_x_px"], st["init_y_px"] = x[pick], y[pick]
    st["theta"] = np.linspace(0.0, 6.0, len(pick)).astype(np.float32)
    st["scale"], st["have_init"] = 1.0, 1
    return st, known[pick]


@pytest.mark.parametrize("kind", ["half", "thirds"])
def test_the_gate_falls_where_the_true_count_says(tdr, oracle, restore, kind):
    """Particles on a line across the edge of the unknown half-plane, among them known counts of P/2 - 1, P/2 and P/2 + 1:
    NaN exactly where 2 * known < P, whatever share of the bins is empty, the same bits as the other two ways — and over the
    scan fractions every outcome of the gate count occurs: settled by the non-empty bins, stopped early, walked to the end."""
    nb, nr = 64, 24
    P = nb * nr
    maps, mask = gate_map(kind)
    om = oracle.OracleMap(maps, mask, 1.0)
    tab = oracle.polar_table(nb, nr, np.float32(2 * np.pi / nb))
    st, known = line_particles(oracle, om, tab, P, 6000, (P - 2, P, P + 2) if kind == "half" else (), 200)
    rig = Rig(tdr, nb, nr, st, maps, mask)
    seen = np.zeros(4, np.int64)
    for frac in ("frac20", "frac50", "frac80", "full", "empty"):
        scan = make_scan(frac, nb, nr, seed=7)
        restore.tdr_profile_enable(2)
        gate_counters(restore)
        new = rig.run(scan, ALL_RAY, split=4)      # (four waves of one workgroup share a particle's count)
        ctr = gate_counters(restore)
        restore.tdr_profile_enable(0)
        assert sum(ctr[:3]) == rig.n, ctr
        assert np.array_equal(new, rig.run(scan, ALL_RAY), equal_nan=True), frac   # (the split the launch chooses itself)
        if frac.startswith("frac"):
            seen += np.asarray(ctr)
        if frac != "empty":        # (an empty scan: 0 / 0 where the gate lets a particle through)
            assert np.array_equal(np.isnan(new), 2 * known < P), frac
        assert np.array_equal(new, rig.run(scan, 0.0), equal_nan=True), frac
        assert np.array_equal(new, rig.run(scan, ALL_RAY, patch=0), equal_nan=True), frac
        ref = oracle.compute_weights(om, tab, nb, nr, scan, 1.0, oracle.make_params(NCLS), st.copy())
        assert np.array_equal(np.isnan(new), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert (np.abs(new[ok] - ref[ok]) <= 1e-5 * np.abs(ref[ok])).all()
    if kind == "half":
        assert (seen[:3] > 0).all() and seen[3] > 0, seen


def test_every_split_gives_the_same_bits(tdr, oracle, restore):
    """1, 2 and 4 waves per particle share the gate count in LDS; 8 do not share a workgroup and count exactly."""
    nb, nr = 64, 24
    P = nb * nr
    maps, mask = gate_map("half")
    om = oracle.OracleMap(maps, mask, 1.0)
    tab = oracle.polar_table(nb, nr, np.float32(2 * np.pi / nb))
    st, known = line_particles(oracle, om, tab, P, 6000, (P - 2, P, P + 2), 96)
    rig = Rig(tdr, nb, nr, st, maps, mask)
    scan = make_scan("frac20", nb, nr, seed=9)
    a = rig.run(scan, 0.0)
    assert np.array_equal(np.isnan(a), 2 * known < P)
    for split in (1, 2, 4, 8):
        restore.tdr_profile_enable(2)
        gate_counters(restore)
        got = rig.run(scan, ALL_RAY, split=split)
        ctr = gate_counters(restore)
        restore.tdr_profile_enable(0)
        assert np.array_equal(a, got, equal_nan=True), f"{split} waves per particle"
        assert sum(ctr[:3]) == rig.n, (split, ctr)
        if split == 8:
            assert ctr[0] == 0 and ctr[1] == 0 and ctr[2] == rig.n, ctr
        else:
            assert ctr[1] > 0, (split, ctr)        # fully known windows, a fifth of the bins non-empty: stopped early


def test_a_mixed_launch_through_the_filter(tdr, oracle, restore):
    """Two ParticleFilter.update steps at a span of 16 (dense particles to the shift-uniform kernel, scattered ones to the
    ray-mapped kernel): the same states and weights with the compact lists as with the ray order."""
    from top_down_renderer_amd import synth
    pkg, k = tdr
    sc = synth.make_scene(synth.Config("mixed", 6000, NCLS, 64, 24, 300, 20480, seed=6300))
    cfg = sc.cfg
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    restore.tdr_config_shift_uniform(2)
    restore.tdr_config_shift_uniform_span(16.0)
    got = []
    for patch in (1, 0):
        restore.tdr_config_tuning(b"ray_patch", patch)
        f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), seed=3, kernels=k, init_particles=False,
                               locality_every=1)
        f.set_states(sc.states)
        launches = int(restore.tdr_shift_uniform_launches())
        for step in range(2):
            f.propagate((0.5, 0.1), 0.01)
            f.update(scan, None, cfg.res)
        k.synchronize()
        assert int(restore.tdr_shift_uniform_launches()) == launches + 2
        got.append((f.get_states().copy(), f.raw_weights().copy(), f.weights().copy()))
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1], got[1][1], equal_nan=True)
    assert np.array_equal(got[0][2], got[1][2], equal_nan=True)
