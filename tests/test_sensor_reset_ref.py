"""CPU-only: the NumPy restatement of sensor resetting (tests/sensor_reset_ref.py) against the restatement of the recovery
injection it extends (tests/recovery_ref.py), and its pick rule on hand-made weight rows."""
import numpy as np
import pytest

import recovery_ref as RR
import sensor_reset_ref as SR

F32 = np.float32
NAN = float("nan")


def _maps(rows=37, cols=53, seed=3):
    rng = np.random.default_rng(seed)
    maps = rng.uniform(0.0, 50.0, (3, rows, cols)).astype(F32)
    maps[1] = np.where(rng.random((rows, cols)) < 0.2, 0.0, 3.0)
    return maps


def _states(n, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros(n, RR.STATE_DTYPE)
    st["init_x_px"], st["init_y_px"] = rng.normal(-300, 40, n), rng.normal(-50, 40, n)
    st["dx_m"], st["dy_m"] = rng.normal(0, 8, n), rng.normal(0, 8, n)
    st["theta"] = rng.uniform(-3, 3, n)
    st["scale"] = np.exp(rng.uniform(-0.3, 1.0, n))
    st["have_init"] = rng.random(n) < 0.9
    return st


CASES = [(300, 0, 9, 5, 1 << 22, 2.0), (65, 1000, (1 << 40) + 3, (1 << 33) + 1, 1 << 23, 1.0), (64, 0, 1, 0, 1 << 24, 1.0),
         (10, 3, 7, 7, 0, 1.0)]


@pytest.mark.parametrize("n,begin,seed,draw,th,res", CASES)
def test_one_candidate_with_a_heading_is_the_plain_injection(n, begin, seed, draw, th, res):
    maps = _maps()
    road = RR.road_cells(maps)
    st = _states(n, n)
    want, cnt = RR.inject(st, n, begin, road, maps.shape[2], res, seed, draw, th, 1)
    got, lst, picks = SR.inject_sensor(st, n, begin, road, maps.shape[2], res, seed, draw, th, 1, 1,
                                       lambda c: (np.ones(len(c), F32), c))
    assert got.tobytes() == want.tobytes() and len(lst) == cnt and (picks == 0).all()
    assert (np.diff(lst) > 0).all()
    if th == 1 << 24:
        assert np.array_equal(lst, np.arange(n))
    if th == 0:
        assert len(lst) == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,begin,seed,draw,th,res", CASES[:3])
def test_candidate_0_is_the_plain_injections_particle(n, begin, seed, draw, th, res, mode):
    maps = _maps()
    road = RR.road_cells(maps)
    st = _states(n, n + 1)
    want, cnt = RR.inject(st, n, begin, road, maps.shape[2], res, seed, draw, th, mode)
    lst = SR.inject_list(n, begin, seed, draw, th)
    cand = SR.candidates(st, lst, 5, begin, road, maps.shape[2], res, seed, draw, mode)
    assert cand.shape == (cnt, 5) and cand[:, 0].tobytes() == want[lst].tobytes()
    # the other candidates: road cells of their own, the slot's scale, no displacement
    assert RR.on_road(maps, res, cand["init_x_px"].ravel(), cand["init_y_px"].ravel()).all()
    assert (cand["scale"] == st["scale"][lst][:, None]).all() and not cand["dx_m"].any() and not cand["dy_m"].any()
    assert (cand["have_init"] == mode).all() and (mode == 1 or not cand["theta"].any())
    if cnt > 3:
        assert (cand["init_x_px"][:, 1:] != cand["init_x_px"][:, :1]).any()
    # a slot's candidates do not depend on how many are asked for
    assert SR.candidates(st, lst, 2, begin, road, maps.shape[2], res, seed, draw, mode).tobytes() == cand[:, :2].tobytes()


def test_the_pick_rule():
    rows = [([1.0, 3.0, 3.0, 2.0], 1),            # ties take the first
            ([NAN, 0.5, NAN, 0.5], 1),            # a NaN is never picked
            ([NAN, NAN, NAN, NAN], 0),            # all NaN: candidate 0
            ([0.0, 0.0, 1e-30, 0.0], 2),          # 0 (gated) loses to a positive weight
            ([0.0, NAN, 0.0, NAN], 0),            # ... and wins against a NaN
            ([NAN, 0.0, 0.0, 0.0], 1),
            ([5.0, 4.0, 3.0, 6.0], 3)]
    w = np.array([r for r, _ in rows], F32)
    assert SR.pick(w).tolist() == [j for _, j in rows]
    assert SR.pick(np.array([[7.0]], F32)).tolist() == [0] and SR.pick(np.array([[NAN]], F32)).tolist() == [0]


def test_the_write_takes_what_scoring_left():
    maps = _maps()
    road = RR.road_cells(maps)
    st = _states(200, 5)

    def score(c):          # a scorer that gives every candidate a heading, like the mode-0 search; the last candidate is best
        after = c.copy()
        after["theta"], after["have_init"] = 0.25, 1
        return np.tile(np.arange(4, dtype=F32), len(c) // 4), after

    got, lst, picks = SR.inject_sensor(st, 200, 0, road, maps.shape[2], 1.0, 3, 4, 1 << 22, 0, 4, score)
    cand = SR.candidates(st, lst, 4, 0, road, maps.shape[2], 1.0, 3, 4, 0)
    assert len(lst) > 10 and (picks == 3).all()
    assert (got["theta"][lst] == F32(0.25)).all() and (got["have_init"][lst] == 1).all()
    assert (got["init_x_px"][lst] == cand["init_x_px"][:, 3]).all()
    rest = np.setdiff1d(np.arange(200), lst)
    assert got[rest].tobytes() == st[rest].tobytes()
