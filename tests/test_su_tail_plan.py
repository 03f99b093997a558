"""The rows of the shift-uniform kernel's grid (su_tail_plan, csrc/tdr_score_su.h, through tdr_su_tail_plan): the last K
ring groups cut into Q sector ranges each.  Whatever K and Q, every (ring group, sector) pair belongs to exactly one row —
that is all the kernel's exact integer sums need to give the same bits.  No GPU."""
import ctypes as C

import pytest

NSECT = 8
NCHUNKS = (1, 2, 3, 32)
PARTS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def lib():
    from top_down_renderer_amd import _lib
    return _lib.load()


def _rows(lib, nchunks, k, q):
    """[(group, s0, s1)] of every row, and the row count the plan reports."""
    R = lib.tdr_su_tail_plan(nchunks, k, q, -1, None, None, None)
    out = []
    for row in range(R):
        g, s0, s1 = C.c_int(-7), C.c_int(-7), C.c_int(-7)
        assert lib.tdr_su_tail_plan(nchunks, k, q, row, C.byref(g), C.byref(s0), C.byref(s1)) == R
        out.append((g.value, s0.value, s1.value))
    return out, R


def _ks(nchunks):
    return sorted({0, 1, nchunks, nchunks + 3})


@pytest.mark.parametrize("nchunks", NCHUNKS)
def test_every_group_sector_pair_is_covered_exactly_once(lib, nchunks):
    for k in _ks(nchunks):
        for q in PARTS:
            rows, _ = _rows(lib, nchunks, k, q)
            seen = {}
            for g, s0, s1 in rows:
                assert 0 <= g < nchunks and 0 <= s0 < s1 <= NSECT, (nchunks, k, q, g, s0, s1)
                for s in range(s0, s1):
                    seen[(g, s)] = seen.get((g, s), 0) + 1
            assert seen == {(g, s): 1 for g in range(nchunks) for s in range(NSECT)}, (nchunks, k, q)


@pytest.mark.parametrize("nchunks", NCHUNKS)
def test_row_count_and_whole_groups_in_front(lib, nchunks):
    for k in _ks(nchunks):
        kk = min(k, nchunks)
        for q in PARTS:
            rows, R = _rows(lib, nchunks, k, q)
            assert R == (nchunks - kk) + kk * q
            # the rows below nchunks - K are whole groups, in order; behind them Q rows of 8 / Q sectors per group, in order
            assert rows[: nchunks - kk] == [(g, 0, NSECT) for g in range(nchunks - kk)]
            w = NSECT // q
            assert rows[nchunks - kk:] == [(g, p * w, (p + 1) * w) for g in range(nchunks - kk, nchunks) for p in range(q)]


@pytest.mark.parametrize("nchunks", NCHUNKS)
def test_no_tail_groups_or_one_part_is_the_identity(lib, nchunks):
    same = [(g, 0, NSECT) for g in range(nchunks)]
    for q in PARTS:
        assert _rows(lib, nchunks, 0, q) == (same, nchunks)
    for k in _ks(nchunks):
        assert _rows(lib, nchunks, k, 1) == (same, nchunks)


def test_rows_outside_the_plan_write_nothing(lib):
    g, s0, s1 = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    for row in (-1, 11, 1 << 20):
        assert lib.tdr_su_tail_plan(4, 1, 8, row, C.byref(g), C.byref(s0), C.byref(s1)) == 11
        assert (g.value, s0.value, s1.value) == (-7, -7, -7)
    # a part count that is none of 1, 2, 4, 8 rounds down to one; a negative K is none
    assert lib.tdr_su_tail_plan(4, 2, 5, -1, None, None, None) == 2 + 2 * 4
    assert lib.tdr_su_tail_plan(4, 2, 0, -1, None, None, None) == 4
    assert lib.tdr_su_tail_plan(4, -3, 8, -1, None, None, None) == 4


def test_the_knobs_answer_a_query_with_the_value_in_force(lib):
    k0, q0 = lib.tdr_config_tuning(b"su_tail_groups", -1), lib.tdr_config_tuning(b"su_tail_parts", -1)
    try:
        assert k0 >= 0 and q0 in PARTS
        assert lib.tdr_config_tuning(b"su_tail_groups", 5) == 5 and lib.tdr_config_tuning(b"su_tail_groups", -1) == 5
        for q, want in ((1, 1), (2, 2), (3, 2), (4, 4), (7, 4), (8, 8), (100, 8), (0, 1)):
            assert lib.tdr_config_tuning(b"su_tail_parts", q) == want
            assert lib.tdr_config_tuning(b"su_tail_parts", -1) == want
    finally:
        lib.tdr_config_tuning(b"su_tail_groups", k0)
        lib.tdr_config_tuning(b"su_tail_parts", q0)
