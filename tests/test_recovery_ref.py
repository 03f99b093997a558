"""CPU: the NumPy restatement of the recovery injection (tests/recovery_ref.py) against published and hand-worked facts,
and the library's host functions against the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import recovery_ref as RR

F32 = np.float32

PHILOX_VECTORS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for c, k, want in PHILOX_VECTORS:
        assert tuple(int(w) for w in RR.philox(c, k)) == want
    # ... and as one vector call: the broadcast form gives the same words
    cs = np.array([v[0] for v in PHILOX_VECTORS], np.uint64).T
    ks = np.array([v[1] for v in PHILOX_VECTORS], np.uint64).T
    got = RR.philox(tuple(cs), tuple(ks))
    assert got.dtype == np.uint32 and [tuple(int(w) for w in got[:, j]) for j in range(3)] == [v[2] for v in PHILOX_VECTORS]


# ---- the hand-worked injection ---------------------------------------------------------------------------------------------------
# A 5 x 5 map of 2 classes at resolution 2; class 1 is 0 on three cells, 3 elsewhere: (r, c) = (0, 3), (2, 1), (4, 4), so the
# road list is {3, 11, 24}.  seed = 0x0123456789ABCDEF: key = {0x89ABCDEF, 0x01234567}; draw = 2^32 + 5: counter words 1, 2 =
# {5, 1}.  With a from-scratch scalar Philox, a = philox({i, 5, 1, 0}, key) of slots 0..3:
#   0: e30f051f 98c7aef8 b5f99284 4aa2187c   a[0] >> 8 = 14880517 >= 2^23: NOT injected
#   1: 7a97c53f 00883e20 9f2c2bce fe2105b2   8034245 < 2^23; (0x00883e20 * 3) >> 32 = 0 -> cell 3 = (0, 3); ux = 0x9f = 159, uy = 0xfe = 254
#   2: 1feb08f8 7a5c7656 010cc0d9 2ccdfe52   2091784 < 2^23; (0x7a5c7656 * 3) >> 32 = 1 -> cell 11 = (2, 1); ux = 1, uy = 0x2c = 44
#   3: 6b0a0f13 133f1cbf eb1a0798 dbbc05ff   7014927 < 2^23; (0x133f1cbf * 3) >> 32 = 0 -> cell 3 = (0, 3); ux = 0xeb = 235, uy = 0xdb = 219
# positions ((c + ux / 256) * 2, (r + uy / 256) * 2), all exact in float32:
#   1: (3 + 159/256) * 2 = 7.2421875, (254/256) * 2 = 1.984375
#   2: (1 + 1/256) * 2 = 2.0078125,   (2 + 44/256) * 2 = 4.34375
#   3: (3 + 235/256) * 2 = 7.8359375, (219/256) * 2 = 1.7109375
# heading_mode 1: b = philox({i, 5, 1, 1}, key), b[0] = 54fb05db, 0173455f, 1650fb84 for slots 1..3, b[0] >> 8 = 5569285, 95045,
# 1462523, and theta = v * 2^-24 * 6.2831855f - 3.1415927f rounded to float32 at every step = the bit patterns below.
HAND_SEED, HAND_DRAW = 0x0123456789ABCDEF, (1 << 32) + 5
HAND_XY = {1: (7.2421875, 1.984375), 2: (2.0078125, 4.34375), 3: (7.8359375, 1.7109375)}
HAND_THETA_BITS = {1: 0xbf87264c, 2: 0xc046c8ab, 3: 0xc02601ed}     # -1.0558562, -3.1059978, -2.5938675


def hand_map():
    maps = np.full((2, 5, 5), 3.0, F32)
    maps[0] = 0.0
    for r, c in ((0, 3), (2, 1), (4, 4)):
        maps[1, r, c] = 0.0
    return maps


def hand_states():
    st = np.zeros(6, RR.STATE_DTYPE)          # 4 slots and two sentinels behind n
    st["init_x_px"] = [100, 101, 102, 103, 104, 105]
    st["init_y_px"] = [200, 201, 202, 203, 204, 205]
    st["dx_m"] = [1, 2, 3, 4, 5, 6]
    st["dy_m"] = [-1, -2, -3, -4, -5, -6]
    st["theta"] = [0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    st["scale"] = [1.5, 1.25, 1.75, 2.0, 3.0, 4.0]
    st["have_init"] = 1
    return st


@pytest.mark.parametrize("mode", [0, 1])
def test_hand_worked_map_and_slots(mode):
    maps = hand_map()
    road = RR.road_cells(maps)
    assert road.tolist() == [3, 11, 24] and road.dtype == np.uint32
    st = hand_states()
    out, cnt = RR.inject(st, 4, 0, road, 5, 2.0, HAND_SEED, HAND_DRAW, 1 << 23, mode)
    assert cnt == 3
    assert out[[0, 4, 5]].tobytes() == st[[0, 4, 5]].tobytes()            # not injected / behind n: every byte as it was
    for i in (1, 2, 3):
        assert (float(out["init_x_px"][i]), float(out["init_y_px"][i])) == HAND_XY[i], i
        assert out["dx_m"][i] == 0 and out["dy_m"][i] == 0
        assert out["scale"][i] == st["scale"][i]                           # the scale stays
        if mode == 0:
            assert out["theta"][i] == 0 and out["have_init"][i] == 0
        else:
            assert int(out["theta"][i:i + 1].view(np.uint32)[0]) == HAND_THETA_BITS[i] and out["have_init"][i] == 1
    assert RR.on_road(maps, 2.0, out["init_x_px"][1:4], out["init_y_px"][1:4]).all()
    # threshold 0: nothing; 2^24: slot 0 too (cell 11 = (2, 1): (0x98c7aef8 * 3) >> 32 = 1; ux = 0xb5 = 181, uy = 0x4a = 74)
    assert RR.inject(st, 4, 0, road, 5, 2.0, HAND_SEED, HAND_DRAW, 0, mode)[0].tobytes() == st.tobytes()
    full, cnt = RR.inject(st, 4, 0, road, 5, 2.0, HAND_SEED, HAND_DRAW, 1 << 24, mode)
    assert cnt == 4 and (float(full["init_x_px"][0]), float(full["init_y_px"][0])) == ((1 + 181 / 256) * 2, (2 + 74 / 256) * 2)
    assert full[1:].tobytes() == out[1:].tobytes()
    # the words of a slot belong to its GLOBAL index: slots 2, 3 as a slice that begins at 2
    part, cnt = RR.inject(st[2:], 2, 2, road, 5, 2.0, HAND_SEED, HAND_DRAW, 1 << 23, mode)
    assert cnt == 2 and part.tobytes() == out[2:].tobytes()


def test_threshold_edges():
    assert RR.threshold(0.0) == 0
    assert RR.threshold(2.0 ** -24) == 1
    assert RR.threshold(2.0 ** -25) == 0
    assert RR.threshold(1.0 - 2.0 ** -24) == (1 << 24) - 1
    assert RR.threshold(1.0) == 1 << 24
    assert RR.threshold(0.5) == 1 << 23
    assert RR.threshold(-0.5) == 0 and RR.threshold(3.0) == 1 << 24 and RR.threshold(float("nan")) == 0


def test_tracker_by_hand():
    """alpha_slow = 1/4, alpha_fast = 1/2, p_max = 1/4; every average is a dyadic number.
      1: w = 8    first update: slow = fast = 8, p = 0
      2: w = 8    slow = 8 + (8 - 8) / 4 = 8, fast = 8, p = 0
      3: w = 4    slow = 8 + (4 - 8) / 4 = 7, fast = 8 + (4 - 8) / 2 = 6, p = 1 - 6/7 = 0.142857 (below p_max)
      4: w = NaN  the state stays, p = 0
      5: w = 1    slow = 7 + (1 - 7) / 4 = 5.5, fast = 6 + (1 - 6) / 2 = 3.5, 1 - 3.5/5.5 = 0.363636 -> p_max = 0.25
      6: w = 16   slow = 5.5 + 10.5 / 4 = 8.125, fast = 3.5 + 12.5 / 2 = 9.75, 1 - 9.75/8.125 < 0 -> 0"""
    t = RR.Tracker(0.25, 0.5, 0.25)
    seen = []
    for w in (8.0, 8.0, 4.0, float("nan"), 1.0, 16.0):
        seen.append((t.track(w), t.w_slow, t.w_fast))
    assert seen == [(0.0, 8.0, 8.0), (0.0, 8.0, 8.0), (1.0 - 6.0 / 7.0, 7.0, 6.0), (0.0, 7.0, 6.0), (0.25, 5.5, 3.5),
                    (0.0, 8.125, 9.75)]
    for w in (0.0, -1.0, float("inf"), float("-inf")):       # non-positive or non-finite: the state stays
        assert t.track(w) == 0.0 and (t.w_slow, t.w_fast) == (8.125, 9.75)
    t.reset()
    assert (t.w_slow, t.w_fast) == (0.0, 0.0)
    assert t.track(3.0) == 0.0 and (t.w_slow, t.w_fast) == (3.0, 3.0)    # the first-update rule again


def test_injected_share_and_cell_histogram():
    """n = 100 003 slots at p = 0.25: the injected count is binomial(n, p), sigma = sqrt(n p (1 - p)) = 136.9; the cells of
    the injected slots are uniform over the 64-cell list: each cell's count is binomial(m, 1/64)."""
    n, p = 100003, 0.25
    road = (np.arange(64, dtype=np.uint32) * 7 + 3)
    st = np.zeros(n, RR.STATE_DTYPE)
    st["init_x_px"] = -1.0
    out, cnt = RR.inject(st, n, 0, road, 1 << 14, 1.0, 20261021, 9, RR.threshold(p), 0)
    assert abs(cnt - n * p) <= 4 * math.sqrt(n * p * (1 - p)), cnt
    sel = out["init_x_px"] >= 0
    assert int(sel.sum()) == cnt
    cells = out["init_x_px"][sel].astype(np.int64)           # resolution 1, one row: the column is the cell index
    assert np.isin(cells, road).all()
    hist = np.array([(cells == c).sum() for c in road])
    sigma = math.sqrt(cnt * (1 / 64) * (63 / 64))
    assert (np.abs(hist - cnt / 64) <= 5 * sigma).all(), hist


# ---- the library's host functions -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from top_down_renderer_amd import _lib, build
    build.build()
    return _lib.load()


def test_host_philox_equals_the_restatement(lib):
    def host(c, k):
        ca, ka, out = (C.c_uint32 * 4)(*c), (C.c_uint32 * 2)(*k), (C.c_uint32 * 4)()
        lib.tdr_philox4x32_host(ca, ka, out)
        return tuple(out)

    for c, k, want in PHILOX_VECTORS:
        assert host(c, k) == want
    rng = np.random.default_rng(3)
    cs = rng.integers(0, 1 << 32, (4, 200), dtype=np.uint64)
    ks = rng.integers(0, 1 << 32, (2, 200), dtype=np.uint64)
    want = RR.philox(tuple(cs), tuple(ks))
    for j in range(200):
        assert host([int(v) for v in cs[:, j]], [int(v) for v in ks[:, j]]) == tuple(int(w) for w in want[:, j])


def test_host_threshold_equals_the_restatement(lib):
    ps = [0.0, 2.0 ** -24, 2.0 ** -25, 1.0 - 2.0 ** -24, 1.0, 0.5, 0.05, 0.25, 1.0 / 3, -0.5, 3.0, float("nan"), float("inf"),
          float("-inf"), np.nextafter(1.0, 0.0), np.nextafter(2.0 ** -24, 0.0)]
    for p in ps:
        assert lib.tdr_inject_threshold_host(C.c_double(p)) == RR.threshold(float(p)), p
    assert lib.tdr_inject_threshold_host(C.c_double(2.0 ** -24)) == 1 and lib.tdr_inject_threshold_host(C.c_double(1.0)) == 1 << 24


def test_host_tracker_equals_the_restatement(lib):
    from top_down_renderer_amd._lib import RecoveryParamsC, RecoveryStateC
    assert C.sizeof(RecoveryStateC) == 16 and C.sizeof(RecoveryParamsC) == 40 and RecoveryParamsC.seed.offset == 32
    rng = np.random.default_rng(4)
    for a_s, a_f, pm in ((0.25, 0.5, 0.25), (0.001, 0.1, 1.0), (1.0, 1.0, 0.5), (0.05, 0.3, 0.0)):
        rp, s, t = RecoveryParamsC(a_s, a_f, pm, 0, 0), RecoveryStateC(0.0, 0.0), RR.Tracker(a_s, a_f, pm)
        ws = [8.0, 8.0, 4.0, float("nan"), 1.0, 16.0, 0.0, -2.0, float("inf")] + list(np.exp(rng.normal(0, 1.5, 60)))
        for i, w in enumerate(ws):
            assert lib.tdr_recovery_track_host(C.byref(s), C.c_double(w), C.byref(rp)) == t.track(w), (i, w)
            assert (s.w_slow, s.w_fast) == (t.w_slow, t.w_fast)
            if i % 17 == 16:
                lib.tdr_recovery_reset_host(C.byref(s))
                t.reset()
                assert (s.w_slow, s.w_fast) == (0.0, 0.0)


def test_job_struct_layout():
    from top_down_renderer_amd._lib import InjectJobC
    assert C.sizeof(InjectJobC) == 88 and InjectJobC.cols.offset == 48 and InjectJobC.seed.offset == 56
    assert InjectJobC.threshold24.offset == 72 and InjectJobC.injected.offset == 80
