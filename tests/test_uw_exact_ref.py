"""tests/uw_exact_ref.py — the exact statement of the update's weights that tests/test_uw_exact.py holds the device to —
against the CPU oracle, against hand-made numbers and against restatements with one mistake each.  No GPU.

(a) the oracle's own weights are one of the candidates, its flag and its argmax the model's, on every committed kind of
    weights and distances: holding the device to the model keeps it inside every tolerance the older tests have against
    the oracle;
(b) four vectors of four weights worked by hand;
(c) the model can fail: a NumPy restatement of the tail is accepted on every case, and rejected on at least one with any
    of five mistakes a kernel could make unseen by a 1e-6 tolerance;
(d) the model is sharp: never more than 4 candidates, and more than one on at most a tenth of the committed cases."""
import numpy as np
import pytest

import uw_exact_ref as X

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("dist", list(X.DISTS))
@pytest.mark.parametrize("kind", list(X.KINDS))
def test_a_oracle_is_a_candidate(oracle, kind, dist):
    for n in X.REF_SIZES:
        raw, ld, cands, fallback, num_valid, num_under, stats = X.model(kind, dist, n)
        with np.errstate(all="ignore"):
            w, best, ostats = oracle.update_weights(raw, ld)
        j = X.match(w, cands)
        assert j >= 0, (n, len(cands))
        assert bool(ostats[3]) == fallback, n
        assert best == X.first_max(cands[j]), n
        assert np.array_equal(np.asarray(ostats[:3], f32), np.asarray(stats, f32), equal_nan=True)


# (b) by hand.  Distances 0.25, 0.125, 0.0625 and 0 give d = min(5 * dist, 1) = 1, 0.625, 0.3125 and 0 without rounding.
def _hand(raw, ld, want_w, want_flag, want_counts, want_stats, want_best):
    raw, ld = np.asarray(raw, f32), np.asarray(ld, f32)
    cands, fallback, num_valid, num_under, stats = X.candidates(raw, ld)
    assert len(cands) == 1                       # every sum below is exact in double and in float
    assert X.same(np.asarray(want_w, f32), cands[0]), (cands[0], want_w)
    assert fallback == want_flag and (num_valid, num_under) == want_counts
    assert np.array_equal(np.asarray(stats, f32), np.asarray(want_stats, f32), equal_nan=True)
    assert X.first_max(cands[0]) == want_best


def test_b_hand_plain():
    # sum = 8, mean = 2; below it 1 and 1: bottom = sqrt((1 + 1) / 2) = 1; no NaN, no fallback
    # w1 = raw / 8 = 1/8, 1/4, 1/2, 1/8;   d = 1, 0.625, 0, 0.3125;   (1 - d) / 4 = 0, 3/32, 1/4, 11/64
    # w2 = 1/8,  5/32 + 3/32 = 1/4,  1/4,  5/128 + 22/128 = 27/128      fs2 = 107/128
    # w  = 16/107, 32/107, 32/107, 27/107 rounded to float: 0x1.323e34p-3, 0x1.323e34p-2 twice, 0x1.02647cp-2;
    # the maximum twice: the first one wins
    _hand([1, 2, 4, 1], [0.25, 0.125, 0, 0.0625],
          [float.fromhex("0x1.323e34p-3"), float.fromhex("0x1.323e34p-2"), float.fromhex("0x1.323e34p-2"),
           float.fromhex("0x1.02647cp-2")], False, (4, 2), (8, 2, 1), 1)


def test_b_hand_fallback_sum_is_zero():
    # sum = 0 over three valid weights: mean = 0, nothing below it, bottom = sqrt(0 / 0) = NaN; the fallback by either clause
    # w0 = 1, fs1 = 4, w1 = 1/4;  w2 = d / 4 + (1 - d) / 4: 1/4;  5/32 + 3/32;  5/64 + 11/64;  1/4     fs2 = 1
    _hand([0, np.nan, 0, 0], [0.25, 0.125, 0.0625, 0], [0.25] * 4, True, (3, 0), (0, 0, np.nan), 0)


def test_b_hand_fallback_nothing_below_the_mean():
    # sum = 8, mean = 2, no weight below 2: num_under = 0 with sum != 0; bottom = sqrt(0 / 0) = NaN
    _hand([2, 2, 2, 2], [0, 0.0625, 0.25, 0.125], [0.25] * 4, True, (4, 0), (8, 2, np.nan), 0)


def test_b_hand_nan_filled():
    # valid 1 and 5: sum = 6, mean = 3; below it 1: bottom = sqrt((1 - 3)^2 / 1) = 2; fill = 3 - 2 = 1
    # w0 = 1, 1, 1, 5; fs1 = 8; w1 = 1/8, 1/8, 1/8, 5/8;   d = 1, 0.625, 0, 0.3125;   (1 - d) / 4 = 0, 3/32, 1/4, 11/64
    # w2 = 16/128,  10/128 + 12/128 = 22/128,  32/128,  25/128 + 22/128 = 47/128      fs2 = 117/128
    # w  = 16/117, 22/117, 32/117, 47/117 rounded to float
    _hand([1, np.nan, np.nan, 5], [0.25, 0.125, 0, 0.0625],
          [float.fromhex("0x1.181182p-3"), float.fromhex("0x1.811812p-3"), float.fromhex("0x1.181182p-2"),
           float.fromhex("0x1.9b59b6p-2")], False, (2, 1), (6, 3, 2), 3)


def test_b_admissible_sums_by_hand():
    # 1 + 2^-24 is the middle between the floats 1 and 1 + 2^-23: a double sum may fall on either side of it
    got = X.admissible_sums(np.asarray([1.0, 2.0 ** -24], f32))
    assert sorted(float(x) for x in got) == [1.0, 1.0 + 2.0 ** -23]
    assert [float(x) for x in X.admissible_sums(np.asarray([1.0, 2.0 ** -23], f32))] == [1.0 + 2.0 ** -23]
    assert [float(x) for x in X.admissible_sums(np.asarray([3e38, 3e38], f32))] == [np.inf]     # finite in double
    assert np.isnan(X.admissible_sums(np.asarray([np.inf, -np.inf, 1.0], f32))[0])
    assert [float(x) for x in X.admissible_sums(np.asarray([-np.inf, 1.0], f32))] == [-np.inf]


# (c) the tail in NumPy, its two sums in index order, and five ways to get it slightly wrong
MISTAKES = ["blend fused", "times the reciprocal of n", "times the reciprocal of fs2", "first sum in float",
            "fill through the counts"]


def _restate(raw, ld, mistake=None):
    n = len(raw)
    stats, num_valid, num_under, fallback = X.chains(raw)
    w0 = X.filled(raw, stats, fallback)
    with np.errstate(all="ignore"):
        if mistake == "first sum in float":
            fs1 = np.cumsum(w0, dtype=f32)[-1]
        elif mistake == "fill through the counts":
            valid_sum = np.sum(raw[~np.isnan(raw)].astype(f64))
            fs1 = f32(f64(n) if fallback else valid_sum + f64(n - num_valid) * f64(f32(stats[1] - stats[2])))
        else:
            fs1 = f32(np.sum(w0.astype(f64)))
        w1 = (w0 / fs1).astype(f32)
        d = np.minimum(ld * f32(5), f32(1))
        if mistake == "blend fused":       # in double, rounded once
            w2 = (d.astype(f64) * w1.astype(f64) + (1.0 - d.astype(f64)) / f64(n)).astype(f32)
        elif mistake == "times the reciprocal of n":
            w2 = ((d * w1).astype(f32) + ((f32(1) - d) * (f32(1) / f32(n))).astype(f32)).astype(f32)
        else:
            w2 = X.blend(w1, ld, n)
        fs2 = f32(np.sum(w2.astype(f64)))
        if mistake == "times the reciprocal of fs2":
            return (w2 * (f32(1) / fs2)).astype(f32)
        return (w2 / fs2).astype(f32)


def _all_cases(sizes):
    return [(kind, dist, n) for kind in X.KINDS for dist in X.DISTS for n in sizes]


def test_c_faithful_restatement_is_accepted_everywhere():
    for key in _all_cases(X.REF_SIZES):
        raw, ld, cands = X.model(*key)[:3]
        assert X.match(_restate(raw, ld), cands) >= 0, key


@pytest.mark.parametrize("mistake", MISTAKES)
def test_c_one_mistake_is_rejected(mistake):
    rejected = []
    for key in _all_cases(X.REF_SIZES):
        raw, ld, cands = X.model(*key)[:3]
        if X.match(_restate(raw, ld, mistake), cands) < 0:
            rejected.append(key)
    print(f"{mistake}: rejected on {len(rejected)} of {len(_all_cases(X.REF_SIZES))} cases")
    assert rejected
    if mistake == "fill through the counts":
        # exactly where nothing is NaN and the fill is not finite: 0 * inf, 0 * NaN
        assert {k[0] for k in rejected} == {"bottom overflows, no nan", "sum overflows"}


def test_d_the_model_is_sharp():
    cases = _all_cases(sorted(set(X.REF_SIZES) | set(X.GPU_SIZES)))
    counts = [len(X.model(*key)[2]) for key in cases]
    multi = sum(c > 1 for c in counts)
    print(f"cases with more than one candidate: {multi} of {len(cases)}; most candidates: {max(counts)}")
    assert min(counts) >= 1 and max(counts) <= 4
    assert multi * 10 <= len(cases)
