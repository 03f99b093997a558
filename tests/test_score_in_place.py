"""The integer form's sums are added IN PLACE (csrc/tdr_score_int_dev.h: int_add_sums, ray_add_sums): every row of
score_polar_su_kernel and every wave of score_polar_ray_kernel adds its share of a slot's class sums (one 64-bit atomic per
class), normalisation and known count into one block that the preparation kernel zeroes in every call, and
score_finalize_exact_kernel reads one row per slot.  Run with `pytest -m gpu`.

  1. every partition of a window — waves per scattered particle, ring groups and tail rows of the dense kernel, the mixed
     launch — gives one set of bits, the oracle's to 1e-5;
  2. nothing is left behind between calls on one workspace (another particle set, fewer particles, another split);
  3. a call that falls back to the float kernels in between (a fractional count) has the plain float launch's bits and leaves
     the integer calls around it alone;
  4. class totals past 2^32 made of rows that each add more than 2^31: the weights are those of the exact sum (Python integers,
     rounded once) — two 32-bit adds on the halves would lose the carry.

The scene of 1-3 is tests/test_finalize_rows.py's, with its tolerance and assertions; 4 takes a launch of
tests/int_form_cases.py."""
import numpy as np
import pytest

import int_exact_ref
import int_form_cases as T

pytestmark = pytest.mark.gpu

N_TOTAL = 1_000_000
ALL_RAY = 1e-6     # span: every particle through the ray-mapped kernel
ALL_DENSE = 1e6    # ... through the shift-uniform kernel
KNOBS = ("su_tail_groups", "su_tail_parts", "su_group")


@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pkg, HipKernels()


class Scene:
    """tests/test_finalize_rows.py's launch: 3000 particles, every ninth moved across the map's border; the oracle's weights."""

    def __init__(self, tdr, oracle):
        from top_down_renderer_amd import synth
        pkg, k = tdr
        sc = synth.make_scene(synth.Config("finrows", 6000, 6, 64, 32, 300, 3000, seed=5177))
        self.cfg = cfg = sc.cfg
        st = sc.states.copy()
        rng = np.random.default_rng(6)
        st["init_x_px"][::9] = rng.uniform(-100, 400, len(st[::9])).astype(np.float32)   # borders, outside: NaN weights too
        self.st = st
        self.m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
        self.m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
        self.scan = oracle.raster_polar(sc.pts, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
        self.ref = oracle.compute_weights(oracle.OracleMap(sc.class_maps, sc.class_mask, 1.0),
                                          oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res), cfg.nb, cfg.nr, self.scan, cfg.res,
                                          oracle.make_params(cfg.ncls, fixed_scale=1.0), st.copy())
        self.ref.setflags(write=False)
        self.pk = self.m.scan_handle(self.scan)

    def filter(self, tdr, st):
        """(filter, locality order) of the particles st"""
        import torch
        pkg, k = tdr
        f = pkg.ParticleFilter(len(st), self.m, pkg.FilterParams(fixed_scale=1.0), kernels=k, init_particles=False, locality_every=1)
        f.set_states(st)
        loc = k.zeros((f.cap_local,), torch.int32)
        k.locality_order(f.st, len(st), self.m.rows, self.m.cols, loc)
        return f, loc

    def score(self, tdr, f, loc, n, pk=None):
        _, k = tdr
        f.raw_w.fill_(-7.0)
        k.score(self.m.dev, self.pk if pk is None else pk, float(self.cfg.res), f.fp_c, f.st, n, f.raw_w, perm=loc,
                uniform_scale=f._uniform_scale, n_total=N_TOTAL, ctx=None)
        k.synchronize()
        return f.raw_w[:n].cpu().numpy()


@pytest.fixture(scope="module")
def scene(tdr, oracle):
    return Scene(tdr, oracle)


@pytest.fixture
def knobs(tdr):
    """Sets tuning knobs by name; the process-wide switches are put back afterwards."""
    _, k = tdr
    before = {n: int(k.lib.tdr_config_tuning(n.encode(), -1)) for n in KNOBS}
    mode = k.lib.tdr_config_shift_uniform(-1)

    def put(**kw):
        for name, v in kw.items():
            assert k.lib.tdr_config_tuning(name.encode(), int(v)) == int(v), name

    yield put
    put(**before)
    k.lib.tdr_config_shift_uniform(mode)
    k.lib.tdr_config_shift_uniform_span(-2.0)
    k.lib.tdr_config_ray_split(0)


def _like_the_oracle(w, ref):
    assert not (w == -7.0).any()
    assert np.array_equal(np.isnan(w), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(w[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    assert err.max(initial=0.0) <= 1e-5, err.max()


def test_every_partition_gives_one_set_of_bits(tdr, scene, knobs):
    _, k = tdr
    n = len(scene.st)
    f, loc = scene.filter(tdr, scene.st)
    k.lib.tdr_config_shift_uniform(2)
    got = {}
    k.lib.tdr_config_shift_uniform_span(ALL_RAY)
    for split in (1, 2, 3, 4, 8):                                # waves, i.e. adders, per scattered slot
        k.lib.tdr_config_ray_split(split)
        got[f"ray-mapped, {split} waves per particle"] = scene.score(tdr, f, loc, n)
    k.lib.tdr_config_ray_split(0)
    k.lib.tdr_config_shift_uniform_span(ALL_DENSE)
    # 32 rings: one group, one row per slot; 4 groups, the last 2 in 4 parts: 10 rows; 8 groups of 8 parts: 64, the most
    for group, tail_k, tail_q in ((32, 0, 1), (8, 2, 4), (4, 1 << 20, 8)):
        knobs(su_group=group, su_tail_groups=tail_k, su_tail_parts=tail_q)
        rows = k.lib.tdr_su_tail_plan((scene.cfg.nr + group - 1) // group, tail_k, tail_q, -1, None, None, None)
        launches = int(k.lib.tdr_shift_uniform_launches())
        got[f"dense, {rows} rows per slot"] = scene.score(tdr, f, loc, n)
        assert int(k.lib.tdr_shift_uniform_launches()) == launches + 1
    assert {"dense, 1 rows per slot", "dense, 10 rows per slot", "dense, 64 rows per slot"} <= set(got)
    knobs(su_group=0, su_tail_groups=4, su_tail_parts=4)
    k.lib.tdr_config_shift_uniform_span(16.0)
    got["mixed launch, span 16"] = scene.score(tdr, f, loc, n)
    first = got["ray-mapped, 1 waves per particle"]
    _like_the_oracle(first, scene.ref)
    for name, w in got.items():
        assert not (w == -7.0).any(), name
        assert np.array_equal(first, w, equal_nan=True), name


def test_nothing_is_left_behind_between_calls(tdr, scene, knobs):
    """A, then B — other particles, fewer of them, another dense / scattered split — then A again, on one filter and one
    workspace; B alone on a fresh filter and a workspace full of a bit pattern that is no sum."""
    import torch
    _, k = tdr
    n_a, n_b = len(scene.st), 1300
    st_b = np.ascontiguousarray(scene.st[::-1])
    k.lib.tdr_config_shift_uniform(2)
    f, loc_a = scene.filter(tdr, scene.st)
    k.lib.tdr_config_shift_uniform_span(16.0)
    a1 = scene.score(tdr, f, loc_a, n_a)
    f.set_states(st_b)
    loc_b = k.zeros((f.cap_local,), torch.int32)
    k.locality_order(f.st, n_b, scene.m.rows, scene.m.cols, loc_b)
    k.lib.tdr_config_shift_uniform_span(4.0)
    b_between = scene.score(tdr, f, loc_b, n_b)
    f.set_states(scene.st)
    k.lib.tdr_config_shift_uniform_span(16.0)
    a2 = scene.score(tdr, f, loc_a, n_a)
    assert np.array_equal(a1, a2, equal_nan=True)
    _like_the_oracle(a1, scene.ref)
    fresh, loc_f = scene.filter(tdr, st_b[:n_b])
    k._workspace(scene.cfg.ncls, scene.cfg.nb, scene.cfg.nr, n_b, N_TOTAL).view(torch.int32).fill_(0x7FC00000)
    k.lib.tdr_config_shift_uniform_span(4.0)
    b_alone = scene.score(tdr, fresh, loc_f, n_b)
    assert np.array_equal(b_between, b_alone, equal_nan=True)
    _like_the_oracle(b_alone, scene.ref[::-1][:n_b])


def test_a_float_fallback_between_two_integer_calls(tdr, scene, knobs):
    """The middle call's scan has a fractional count: the device raises `inexact`, the float kernels write and read their own
    rows of the same workspace — the plain float launch's bits — and the integer calls around it do not notice."""
    _, k = tdr
    n = len(scene.st)
    frac = scene.scan.copy()
    occupied = np.flatnonzero(frac.sum(axis=0) > 0)
    frac[1, occupied[len(occupied) // 2]] += 0.5
    pk_frac = scene.m.scan_handle(frac)
    f, loc = scene.filter(tdr, scene.st)
    k.lib.tdr_config_shift_uniform_span(16.0)
    k.lib.tdr_config_shift_uniform(0)
    plain = scene.score(tdr, f, loc, n, pk=pk_frac)
    k.lib.tdr_config_shift_uniform(2)
    first = scene.score(tdr, f, loc, n)
    fallback = scene.score(tdr, f, loc, n, pk=pk_frac)
    second = scene.score(tdr, f, loc, n)
    assert not (fallback == -7.0).any()
    assert np.array_equal(fallback, plain, equal_nan=True)
    assert np.array_equal(first, second, equal_nan=True)
    _like_the_oracle(first, scene.ref)
    assert not np.array_equal(first, fallback, equal_nan=True)   # (the fractional count is part of the middle call's weights)


def _share_totals(case, oracle, st, share_of_bin, cls):
    """Per share of particle st's window (share_of_bin[k]: the share scan bin k belongs to): class cls's sum count x value 2^q
    as Python integers."""
    q = int_exact_ref.map_power(case["maps"])
    dists, _, src = T.window_of(oracle, case, st)
    counts = case["scan"][cls].astype(np.uint64)
    vints = np.ldexp(dists[cls, src].astype(np.float64), q).astype(np.uint64)
    out = {}
    for s in np.unique(share_of_bin):
        sel = share_of_bin == s
        out[int(s)] = int_exact_ref.exact_dot(counts[sel], vints[sel])
    return out


def test_the_carry_between_the_halves(tdr, oracle, knobs):
    """tests/int_form_cases.py, "class_sum_past_2p53": one class with counts in the millions, every total far past 2^32.  The
    rows of a slot — ring groups of the dense kernel, direction shares of the ray-mapped one — each add more than 2^31, so
    the low halves carry; the weights are the exact sum's, bit for bit."""
    import torch
    pkg, k = tdr
    case, exact, _ = T.references(oracle, "class_sum_past_2p53", "polar")
    nb, nr = case["shape"]
    cls, total = case["made_total"]
    st = case["states"]
    group, split = 4, 8
    # what the launches below partition particle 0's window into: the rings' groups; the waves' shares of the window's directions
    ring, a = np.arange(nb * nr) // nb, np.arange(nb * nr) % nb
    shift = oracle.rot_shift(float(st[0]["theta"]), nb)
    per = (nb + split - 1) // split
    for shares in (_share_totals(case, oracle, st[0], ring // group, cls),
                   _share_totals(case, oracle, st[0], ((a - shift) % nb) // per, cls)):
        assert sum(shares.values()) == total and total > 2 ** 32
        assert sum(1 for v in shares.values() if v > 2 ** 31) >= 2, shares
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), case["maps"], case["mask"], kernels=k)
    m.samplePtsPolar((nb, nr), case["ang_res"])
    f = pkg.ParticleFilter(len(st), m, pkg.FilterParams(**case["params"]), kernels=k, init_particles=False, locality_every=1)
    f.set_states(st)
    loc = k.zeros((f.cap_local,), torch.int32)
    k.locality_order(f.st, len(st), m.rows, m.cols, loc)
    pk = m.scan_handle(case["scan"])
    k.lib.tdr_config_shift_uniform(2)
    knobs(su_group=group, su_tail_groups=2, su_tail_parts=4)
    k.lib.tdr_config_ray_split(split)
    for span in (ALL_DENSE, 3.0, ALL_RAY):
        k.lib.tdr_config_shift_uniform_span(span)
        f.raw_w.fill_(-7.0)
        k.score(m.dev, pk, float(case["res"]), f.fp_c, f.st, len(st), f.raw_w, perm=loc, uniform_scale=f._uniform_scale,
                n_total=N_TOTAL, ctx=None)
        k.synchronize()
        w = f.raw_w[:len(st)].cpu().numpy()
        assert np.array_equal(np.isnan(w), np.isnan(exact)), span
        ok = ~np.isnan(exact)
        assert (w[ok] == exact[ok]).all(), (span, int((w[ok] != exact[ok]).sum()))
