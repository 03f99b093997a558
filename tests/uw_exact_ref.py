"""The exact statement of ParticleFilter::update's weights (particle_filter.cpp:107-147) that tdr_k_update_weights is held to
on every path (tests/test_uw_exact.py), and the weights and travel distances it is held to it on.  Checked against the CPU
oracle and hand-made numbers in tests/test_uw_exact_ref.py.  No GPU here.

The update is a fixed sequence of correctly rounded float operations (the library is built with -ffp-contract=off) but for
two sums that the reference leaves to Eigen, `weights_.sum()` in front of either normalisation.  The device takes both in
double, in an order of its own, and rounds to float once.  So its weights are one of a handful of arrays that can be
written down:

  sum, mean, bottom_stddev   the oracle's serial float chains (proven serial elsewhere: test_gpu_parity.py,
                             test_update_chain_launches.py), the two counts from NumPy
  fallback                   sum == 0 or num_under < 1                                                          (:129)
  w0                         all ones in the fallback, else the raw weights with float(mean - bottom) for every NaN  (:130-134)
  fs1                        ANY float a double sum of w0 may round to (admissible_sums)
  w1 = w0 / fs1                                                                                               (:135)
  d  = min(last_dist * 5, 1);  w2 = fl(d * w1) + fl(fl(1 - d) / float(n))    each operation rounded, none fused    (:138-141)
  fs2                        ANY float a double sum of w2 may round to
  w  = w2 / fs2                                                                                               (:142)

At most two values of fs1 times two of fs2 in practice: candidates() returns them all, and an output matches a candidate when
its NaNs sit where the candidate's do and every other element has the candidate's 32 bits (NaN payloads are free).

Domain: last_dist is finite and >= 0, which is all a propagate produces.  For a NaN distance the reference's
std::min<float>(NaN, 1) is NaN and the kernels' fminf(NaN, 1) is 1: outside the contract, and not tested."""
import math

import numpy as np

f32 = np.float32
f64 = np.float64


def _oracle():
    from oracle import c_oracle

    return c_oracle


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(out, cand):
    """The comparison rule: NaN where the candidate has NaN, the candidate's bits everywhere else."""
    out, cand = np.asarray(out, f32), np.asarray(cand, f32)
    if out.shape != cand.shape:
        return False
    nan = np.isnan(cand)
    return bool(np.array_equal(np.isnan(out), nan) and np.array_equal(_bits(out)[~nan], _bits(cand)[~nan]))


def match(out, cands):
    """Index of the first candidate `out` matches, or -1."""
    for j, c in enumerate(cands):
        if same(out, c):
            return j
    return -1


def first_max(w):
    """:145-147 as the device states it: the largest weight, the smallest index among equals; a NaN never wins; 0 if every
    weight is NaN."""
    w = np.asarray(w, f32)
    ok = np.flatnonzero(~np.isnan(w))
    return int(ok[np.argmax(w[ok])]) if len(ok) else 0


def admissible_sums(v):
    """The floats a double sum of the float array v may round to, whatever the order of the additions.

    With a NaN or an infinity among the addends the order does not matter (no partial sum of finite floats overflows a
    double): the one value NumPy's sum gives.  Otherwise a sum of m doubles in any order is within (m - 1) 2^-53 sum|v| of
    the exact sum S, to first order; (m + 1) 2^-53 sum|v| covers the higher orders with room to spare, and the set is what
    S - bound, S and S + bound round to: one value, or two where S lies that close to the middle between two floats."""
    v = np.asarray(v, f32).astype(f64)
    with np.errstate(all="ignore"):
        if not np.all(np.isfinite(v)):
            return [f32(np.sum(v))]
        s = math.fsum(v.tolist())
        bound = (len(v) + 1) * 2.0 ** -53 * math.fsum(np.abs(v).tolist())
        out = []
        for x in (s - bound, s, s + bound):
            fx = f32(x)
            if not any(_bits(fx) == _bits(o) for o in out):
                out.append(fx)
    return out


def chains(raw):
    """(sum, mean, bottom_stddev) from the oracle's serial chains, the valid count, the count below the mean, the flag."""
    raw = np.ascontiguousarray(raw, f32)
    with np.errstate(all="ignore"):
        _, _, stats = _oracle().update_weights(raw, np.zeros(len(raw), f32))
        s, mean, bottom = f32(stats[0]), f32(stats[1]), f32(stats[2])
        num_valid = int(np.count_nonzero(~np.isnan(raw)))
        num_under = int(np.count_nonzero(raw < mean))   # a NaN on either side compares false
    fallback = bool(s == 0 or num_under < 1)
    return (s, mean, bottom), num_valid, num_under, fallback


def filled(raw, stats, fallback):
    """w0: :130 or :133-134."""
    raw = np.asarray(raw, f32)
    if fallback:
        return np.ones(len(raw), f32)
    with np.errstate(all="ignore"):
        fill = f32(stats[1] - stats[2])
    return np.where(np.isnan(raw), fill, raw).astype(f32)


def blend(w1, last_dist, n):
    """:138-141, every operation rounded to float on its own."""
    with np.errstate(all="ignore"):
        d = np.minimum(np.asarray(last_dist, f32) * f32(5), f32(1))
        a = (d * w1).astype(f32)
        b = ((f32(1) - d) / f32(n)).astype(f32)
        return (a + b).astype(f32)


def candidates(raw, last_dist):
    """(list of weight arrays, fallback, num_valid, num_under, (sum, mean, bottom)) for one call of the update."""
    raw = np.ascontiguousarray(raw, f32)
    last_dist = np.ascontiguousarray(last_dist, f32)
    n = len(raw)
    stats, num_valid, num_under, fallback = chains(raw)
    w0 = filled(raw, stats, fallback)
    out = []
    with np.errstate(all="ignore"):
        for fs1 in admissible_sums(w0):
            w2 = blend((w0 / fs1).astype(f32), last_dist, n)
            for fs2 in admissible_sums(w2):
                c = (w2 / fs2).astype(f32)
                if match(c, out) < 0:
                    out.append(c)
    return out, fallback, num_valid, num_under, stats


# ---- the weights and the travel distances of the committed cases -----------------------------------------------------------

def _lognormal(n, rng):
    raw = np.exp(rng.normal(0, 3, n)).astype(f32)
    raw[rng.random(n) < 0.02] = np.nan
    return raw


def _zeros_and_nan(n, rng):       # sum == 0: the fallback
    raw = np.zeros(n, f32)
    raw[rng.random(n) < 0.3] = np.nan
    return raw


def _all_nan(n, rng):
    return np.full(n, np.nan, f32)


def _one_valid(n, rng):           # the mean is the one weight: nothing below it
    raw = np.full(n, np.nan, f32)
    raw[n // 3] = f32(2.5)
    return raw


def _equal(n, rng):               # the float sum of n ones is exact and the mean 1: no weight below it, the fallback
    return np.full(n, f32(1.0), f32)


def _three_values(n, rng):        # exact ties in bulk
    return np.asarray([0.5, 1.25, 3.0], f32)[rng.integers(0, 3, n)]


def _bottom_overflows(n, rng):    # (v - mean)^2 is past the float range for every weight below the mean: bottom = inf
    raw = (rng.random(n) + 0.5).astype(f32)
    raw[0] = f32(3e38)
    return raw


def _bottom_overflows_nan(n, rng):   # ... and a NaN to fill with mean - inf
    raw = _bottom_overflows(n, rng)
    raw[n // 2] = np.nan
    return raw


def _sum_overflows(n, rng):       # sum = mean = bottom = inf from the second weight on, fill = NaN, nothing to fill
    raw = np.full(n, f32(3e38), f32)
    raw[::3] = f32(1e38)
    return raw


def _inf_inside(n, rng):
    raw = (rng.random(n) + 0.25).astype(f32)
    raw[n // 3] = np.inf
    return raw


def _subnormal(n, rng):
    raw = (rng.random(n) * 1e-41).astype(f32)
    raw[rng.random(n) < 0.05] = np.nan
    return raw


def _negative(n, rng):            # the fill and some weights come out negative
    raw = (rng.random(n) - 0.3).astype(f32)
    raw[rng.random(n) < 0.05] = np.nan
    return raw


KINDS = {
    "lognormal": _lognormal,
    "zeros and nan": _zeros_and_nan,
    "all nan": _all_nan,
    "one valid": _one_valid,
    "equal power of two": _equal,
    "three values": _three_values,
    "bottom overflows, no nan": _bottom_overflows,
    "bottom overflows, one nan": _bottom_overflows_nan,
    "sum overflows": _sum_overflows,
    "inf inside": _inf_inside,
    "subnormal": _subnormal,
    "negative": _negative,
}


def _dist_random(n, rng):
    ld = (rng.random(n) * 0.4).astype(f32)
    # d = 1 exactly reached; the last d below 1 (fl(5 * 0.19999999) = 1 - 2^-24); a subnormal distance
    first = np.asarray([0.2, np.nextafter(f32(0.2), f32(0)), 1e-40], f32)
    ld[:min(n, 3)] = first[:min(n, 3)]
    return ld


def _dist_zero(n, rng):           # d = 0: every weight becomes 1 / float(n)
    return np.zeros(n, f32)


def _dist_saturated(n, rng):      # d = 1: the weights pass through
    return np.full(n, f32(0.2), f32)


DISTS = {"random": _dist_random, "zero": _dist_zero, "saturated": _dist_saturated}

# the sizes of the CPU comparison with the oracle (tests/test_uw_exact_ref.py)
REF_SIZES = (1, 2, 63, 513, 4097, 20_000, 32_768, 40_000)
# the sizes of the device test (tests/test_uw_exact.py): around a wave (64), a wave-chunk and the <false> workgroup (512), the
# <true> workgroup (1024), a chain chunk (4096), the blend loop's stride (16 x 1024), the reference's operating point, the
# last one-workgroup sizes; above, the first multi-workgroup size (uw_chunk leaves trailing workgroups empty), a last chain
# chunk of one weight, 256 workgroups x 256 threads exactly and one past, a ragged size
GPU_SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 16_383, 16_384, 16_385, 20_000, 32_767,
             32_768, 32_769, 36_865, 65_536, 65_537, 100_003)


def make_case(kind, dist, n):
    """(raw, last_dist) of the committed case: a function of its three names only."""
    kinds, dists = list(KINDS), list(DISTS)
    rng = np.random.default_rng([kinds.index(kind), dists.index(dist), n])
    raw = KINDS[kind](n, rng)
    ld = DISTS[dist](n, rng)
    return np.ascontiguousarray(raw, f32), np.ascontiguousarray(ld, f32)


_MODEL = {}


def model(kind, dist, n):
    """(raw, last_dist) + candidates(raw, last_dist) of a committed case, computed once per process and left unchanged."""
    key = (kind, dist, n)
    if key not in _MODEL:
        raw, ld = make_case(kind, dist, n)
        got = (raw, ld) + candidates(raw, ld)
        for a in (raw, ld) + tuple(got[2]):
            a.setflags(write=False)
        _MODEL[key] = got
    return _MODEL[key]
