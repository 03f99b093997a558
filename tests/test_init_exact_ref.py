"""tests/init_exact_ref.py and the scenes of tests/init_scenes.py on the CPU: the exact search agrees with the oracle
wherever candidates do not tie, every scene pins the heading of at least 90 % of its searched particles, and the rules of
check_choice (first of a shift class, the NaN and zero-denominator branches) on hand-made cases."""
import math

import numpy as np
import pytest

import init_exact_ref as X
import init_scenes as S
from oracle import np_oracle

f32 = np.float32


@pytest.mark.parametrize("key", S.REF_KEYS, ids=lambda k: "-".join(str(x) for x in k))
def test_scene_is_fair_and_agrees_with_the_oracle(oracle, key):
    ref = S.reference(oracle, *key)
    se, st, st_o = ref["search"], ref["st"], ref["st_o"]
    kinds = np.bincount(se.kind, minlength=3)
    print(f"{key}: gated / no winner / searched {kinds}, batches with work {se.wanted_batches()}")
    assert kinds[X.GATED] >= 10 and kinds[X.ALL_NAN] >= 1 and kinds[X.SEARCHED] >= 40
    assert se.wanted_batches() == (3 if se.n == 200 else 1)         # (a whole batch has nothing to do, where there are four)
    idx = se.searched()
    sep = se.separated()
    print(f"{key}: best class separated by more than {X.TAU}: {sep.mean():.3f} of {len(idx)}")
    assert sep.mean() >= 0.9, "the scene pins too few headings"
    # the oracle's float search picks the exact argmin wherever the classes are separated; elsewhere it passes check_choice
    mine = se.thetas[se.best[idx]]
    assert np.array_equal(st_o["theta"][idx][sep].view(np.uint32), mine[sep].view(np.uint32))
    X.check_choice(se, st["theta"], st_o["theta"], st_o["have_init"], ref["raw_o"], ref["raw_o"], st["have_init"])
    # what the oracle leaves alone, the exact search calls gated; a particle nobody can win is at theta 0
    assert np.array_equal(st_o["have_init"] == st["have_init"], se.kind == X.GATED)
    nan = se.kind == X.ALL_NAN
    want = f32(1.0 / (float(X.FLT_MAX) + float(f32(ref["params"]["regularization"]))))
    assert (st_o["theta"][nan] == 0).all() and (ref["raw_o"][nan] == want).all() and want > 0
    if key[2] in ("c2048", "c2049", "sum2200"):
        s = ref["scan"]
        top, tot = s.max(), s.sum(0).max()
        assert (top, tot) == {"c2048": (2048, 2048), "c2049": (2049, 2049), "sum2200": (1100, 2200)}[key[2]]


def test_numpy_oracle_agrees_on_a_small_scene(oracle):
    """np_oracle.compute_weights (the plain restatement) picks the helper's argmin too, wherever the classes are separated."""
    ref = S.reference(oracle, "c3_36x7", "fixed", "plain", "w", 1.0)
    cfg, sc, se, st = ref["cfg"], ref["sc"], ref["search"], ref["st"]
    idx = se.searched()[:40]
    sub = st[idx]
    states = dict(init_x=sub["init_x_px"].copy(), init_y=sub["init_y_px"].copy(), dx=sub["dx_m"].copy(), dy=sub["dy_m"].copy(),
                  theta=sub["theta"].copy(), scale=sub["scale"].copy(), have_init=sub["have_init"].copy())
    fp = dict(ref["params"], scale_log_min=-0.1, scale_log_max=1.0)
    tab = np_oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, 1.0)
    np_oracle.compute_weights(sc.class_maps, sc.class_mask, 1.0, tab, cfg.nb, cfg.nr, ref["scan"], cfg.res, fp, states)
    sep = se.separated()[:40]
    assert sep.sum() >= 30
    assert np.array_equal(states["theta"][sep].view(np.uint32), se.thetas[se.best[idx]][sep].view(np.uint32))
    assert [np_oracle.rot_shift(t, cfg.nb) for t in se.thetas] == [oracle.rot_shift(float(t), cfg.nb) for t in se.thetas]


# ---- hand cases: nb = 8, five candidates per shift ---------------------------------------------------------------------------
def _hand(oracle, scan_of, mask=None, n=1, regularization=0.7):
    nb, nr, ncls, size = 8, 2, 2, 33
    maps = np.empty((ncls, size, size), f32)
    # class 0: grows with x, a little with y — one direction of the window is nearest
    maps[0] = np.arange(size, dtype=f32)[None, :] + 1 + 0.25 * np.arange(size, dtype=f32)[:, None]
    maps[1] = 5
    mask = np.zeros((size, size), np.uint8) if mask is None else mask
    maps[:, mask != 0] = 0
    tab = oracle.polar_table(nb, nr, f32(2 * math.pi / nb), 1.0)
    st = np.zeros(n, oracle.STATE_DTYPE)
    st["init_x_px"], st["init_y_px"], st["scale"] = 16, 16, 1
    fp = oracle.make_params(ncls, class_weights=[1.0, 0.5], regularization=regularization)
    om = oracle.OracleMap(maps, mask, 1.0)
    dists, m = oracle.local_map_polar(om, tab, f32(16), f32(16), f32(1), 4.0)
    scan = scan_of(dists.reshape(ncls, nr, nb), nb, nr)
    se = X.Search(oracle, maps, mask, 1.0, tab, nb, nr, scan.reshape(ncls, nb * nr), 4.0, fp, st)
    st_o = st.copy()
    raw_o = oracle.compute_weights(om, tab, nb, nr, scan.reshape(ncls, nb * nr), 4.0, fp, st_o)
    return se, st, st_o, raw_o


def test_hand_case_first_of_class(oracle):
    want_shift = 3

    def scan_of(d, nb, nr):
        i_min = int(np.argmin(d[0, 1]))
        assert (d[0, 1] == d[0, 1, i_min]).sum() == 1           # one nearest direction on the outer ring
        s = np.zeros((2, nr, nb), f32)
        s[0, 1, (i_min + want_shift) % nb] = 7                    # pairs with it at shift 3 alone
        return s

    se, st, st_o, raw_o = _hand(oracle, scan_of)
    assert len(se.thetas) == 40 and np.bincount(se.shifts).tolist() == [5] * 8
    members = np.flatnonzero(se.shifts == want_shift)
    assert se.kind[0] == X.SEARCHED and se.best[0] == members[0] and members[0] > 0
    assert len(set(se.cost64[0][members])) == 1 and (se.cost64[0][se.shifts != want_shift] > se.cost64[0][members[0]]).all()
    assert st_o["theta"][0].tobytes() == se.thetas[members[0]].tobytes()          # the reference keeps the first
    ok = lambda theta: X.check_choice(se, st["theta"], np.asarray([theta], f32), np.ones(1, np.uint8), raw_o, raw_o,
                                      st["have_init"])
    assert ok(se.thetas[members[0]]) == 0.0
    for later in members[1:]:                                                      # the same cost, not the first: refused
        with pytest.raises(AssertionError, match="not the first of its shift class"):
            ok(se.thetas[later])
    with pytest.raises(AssertionError, match="exceeds the minimum"):               # the first of another class: dearer
        ok(se.thetas[np.flatnonzero(se.shifts == want_shift + 1)[0]])
    with pytest.raises(AssertionError, match="none of the candidates"):
        ok(np.nextafter(se.thetas[members[0]], f32(7)))
    with pytest.raises(AssertionError, match="was not initialised"):
        X.check_choice(se, st["theta"], se.thetas[members[:1]], np.zeros(1, np.uint8), raw_o, raw_o, st["have_init"])


def test_hand_case_nan_and_zero_denominator(oracle):
    def one(d, nb, nr):                                # one scan point, on the outer ring
        s = np.zeros((2, nr, nb), f32)
        s[0, 1, 0] = 1
        return s

    want = f32(1.0 / (float(X.FLT_MAX) + float(f32(0.7))))
    # fewer than half of the cells known: NaN for every candidate (:117-120), theta stays 0, weight 1 / (FLT_MAX + reg)
    mask = np.ones((33, 33), np.uint8)
    mask[:, :14] = 0
    se, st, st_o, raw_o = _hand(oracle, one, mask=mask)
    assert se.kind[0] == X.ALL_NAN and st_o["theta"][0] == 0 and st_o["have_init"][0] == 1 and raw_o[0] == want
    X.check_choice(se, st["theta"], st_o["theta"], st_o["have_init"], raw_o, raw_o, st["have_init"])
    with pytest.raises(AssertionError, match="theta must stay 0"):
        X.check_choice(se, st["theta"], se.thetas[3:4], st_o["have_init"], raw_o, raw_o, st["have_init"])
    # an empty scan: 0 / 0 for every candidate
    se, st, st_o, raw_o = _hand(oracle, lambda d, nb, nr: np.zeros((2, nr, nb), f32))
    assert se.kind[0] == X.ALL_NAN and st_o["theta"][0] == 0 and raw_o[0] == want
    # the one scan point meets an unknown cell at some shifts (x / 0: cannot win) and a known one at others
    mask = np.zeros((33, 33), np.uint8)
    mask[:, 17:] = 1                                   # the half of the window towards +x is unknown ...
    mask[0:16, 17:] = 0                                # ... but for a quarter: more than half of the cells stay known
    se, st, st_o, raw_o = _hand(oracle, one, mask=mask)
    c = se.cost64[0]
    assert se.kind[0] == X.SEARCHED and np.isinf(c).any() and np.isfinite(c).any()
    assert st_o["theta"][0].tobytes() == se.thetas[se.best[0]].tobytes()
    X.check_choice(se, st["theta"], st_o["theta"], st_o["have_init"], raw_o, raw_o, st["have_init"])
    with pytest.raises(AssertionError, match="exceeds the minimum"):
        X.check_choice(se, st["theta"], se.thetas[np.flatnonzero(np.isinf(c) & se.first)[:1]], st_o["have_init"], raw_o, raw_o,
                       st["have_init"])


def test_gated_particles_are_left_alone(oracle):
    ref = S.reference(oracle, "c6", "pscale", "plain", "w", 1.0)
    se, st, st_o = ref["search"], ref["st"], ref["st_o"]
    gated_uninit = (se.kind == X.GATED) & (st["have_init"] == 0)
    assert gated_uninit.sum() >= 20 and (ref["raw_o"][gated_uninit] == 0).all() and (st_o["have_init"][gated_uninit] == 0).all()
    assert (se.kind[20:26] == [X.GATED, X.GATED] + [se.kind[22], se.kind[23]] + [X.GATED, X.GATED]).all()   # 0.3, 0.79 | 10.5, 12
    assert se.kind[22] != X.GATED and se.kind[23] != X.GATED                                                # 0.8, 10.0
    moved = st_o["theta"].copy()
    p = int(np.flatnonzero(gated_uninit)[0])
    moved[p] = 1.0
    with pytest.raises(AssertionError, match="untouched particle moved"):
        X.check_choice(se, st["theta"], moved, st_o["have_init"], ref["raw_o"], ref["raw_o"], st["have_init"])


@pytest.mark.parametrize("scene", ["c6_8x16", "c11_8x16"])
def test_nb8_scenes_tie_across_the_lanes(oracle, scene):
    """What the nb = 8 rows are for: in the matrix-core kernels the four lanes of a particle hold candidates 16 T + 4 q + r,
    so of the shift classes {13..17} and {28..32} the FIRST member sits in lane 3 and later ones in lane 0 — the one place
    where the cross-lane reduction needs its `equal cost, lower index` term.  (With nb = 36 the shared pairs are (5, 6),
    (14, 15), (25, 26), (35, 36): the earlier member is never in a higher lane.)  Enough particles must choose them."""
    se = S.reference(oracle, scene)["search"]
    for first in (13, 28):
        members = np.flatnonzero(se.shifts == se.shifts[first])
        assert members.tolist() == list(range(first, first + 5)) and se.first[first]
        assert (se.best[se.searched()] == first).sum() >= 5
    se36 = S.reference(oracle, "c6_36x7")["search"]
    assert np.flatnonzero(~se36.first).tolist() == [6, 15, 26, 36]
