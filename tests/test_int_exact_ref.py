"""tests/int_exact_ref.py — the exact statement of the raw weight that the integer form of a scoring launch is held to
(tests/test_int_form_limits.py) — against the CPU oracle and against hand-made numbers.  No GPU.

(a) where every sum is exact in float anyway (maps of small dyadic values, small counts) the exact reference IS the oracle,
    bit for bit.  The oracle adds a class's two blocks (scan rows below the shift, the others: state_particle.cpp:136-139)
    to the cost one after the other, the integer form adds their exact total once: the same bits where one block is empty.
    Cartesian windows have no shift (one block); the polar scans here keep one block empty for every particle while the
    shift still decides which window row a scan row meets.
(b) on EVERY case of the GPU file the oracle stays within 1e-5 (relative) of the exact reference, with its NaN and zero
    pattern: only then does holding the device to the exact reference keep the GPU tests' tolerance against the oracle.
    The table's "integer" / "float" is what the device's own rules give on the host.
(c) the rounding routine on hand-made ties."""
import numpy as np
import pytest

import int_exact_ref as X
import int_form_cases as T

f32 = np.float32


def _bits(w):
    return np.asarray(w, f32).view(np.uint32)


def _dyadic_scene(rng, size=96):
    vals = np.asarray([0.25, 0.5, 1.0, 1.5, 2.75, 6.0, 12.5, 40.0], f32)
    maps = np.kron(vals[rng.integers(0, len(vals), (4, size // 4, size // 4))], np.ones((4, 4), f32)).astype(f32)
    mask = np.zeros((size, size), np.uint8)
    mask[10:30, 50:80] = 1
    maps[:, mask == 1] = 0
    return maps, mask


def _states(oracle, rng, n, size):
    st = np.zeros(n, oracle.STATE_DTYPE)
    st["init_x_px"] = rng.uniform(-10, size + 10, n)
    st["init_y_px"] = rng.uniform(-10, size + 10, n)
    st["dx_m"], st["dy_m"] = rng.normal(0, 2, n), rng.normal(0, 2, n)
    st["scale"] = rng.uniform(0.8, 1.3, n)
    st["have_init"] = 1
    return st


@pytest.mark.parametrize("block", ["rows at and past the shift", "rows below the shift"])
def test_a_exact_reference_is_the_oracle_where_floats_are_exact_polar(oracle, block):
    rng = np.random.default_rng(11)
    nb, nr, n = 24, 10, 64
    maps, mask = _dyadic_scene(rng)
    st = _states(oracle, rng, n, maps.shape[1])
    ang = f32(2 * np.pi / nb)
    scan = np.zeros((4, nr, nb), f32)
    if block == "rows at and past the shift":        # scan rows nb/2..: shifts 0..nb/2 leave the block below the shift empty
        scan[:, :, nb // 2:] = rng.integers(0, 4, (4, nr, nb // 2)) * (rng.random((4, nr, nb // 2)) < 0.4)
        shifts = rng.integers(0, nb // 2 + 1, n)
    else:                                            # scan rows 0..nb/4-1: shifts nb/4.. leave the other block empty
        scan[:, :, :nb // 4] = rng.integers(0, 4, (4, nr, nb // 4)) * (rng.random((4, nr, nb // 4)) < 0.4)
        shifts = rng.integers(nb // 4, nb, n)
    st["theta"] = (shifts * float(ang) + rng.uniform(-0.3, 0.3, n) * float(ang) + 2 * np.pi * rng.integers(-2, 3, n)).astype(f32)
    assert len({oracle.rot_shift(float(t), nb) for t in st["theta"]}) > 5
    scan = scan.reshape(4, nr * nb)
    tab = oracle.polar_table(nb, nr, ang)
    for params in (dict(fixed_scale=1.0), dict(fixed_scale=-1.0, force_on_map=True, class_weights=[1.0, 0.5, 2.0, 0.75])):
        fp = oracle.make_params(4, **params)
        with np.errstate(all="ignore"):
            ref = oracle.compute_weights(oracle.OracleMap(maps, mask, 1.0), tab, nb, nr, scan, 1.0, fp, st.copy())
        got = X.weights_polar(oracle, maps, mask, 1.0, tab, nb, nr, scan, 1.0, fp, st)
        assert np.array_equal(_bits(got), _bits(ref))
        assert np.isnan(ref).any() and (ref > 0).sum() > n // 3
    assert (ref == 0).any()   # the gates


def test_a_exact_reference_is_the_oracle_where_floats_are_exact_cartesian(oracle):
    rng = np.random.default_rng(12)
    rows, cols, n = 20, 12, 64
    maps, mask = _dyadic_scene(rng)
    st = _states(oracle, rng, n, maps.shape[1])
    st["theta"] = rng.uniform(-7, 7, n)
    scan = (rng.integers(0, 4, (4, rows * cols)) * (rng.random((4, rows * cols)) < 0.4)).astype(f32)
    fp = oracle.make_params(4, class_weights=[1.0, 0.5, 2.0, 0.75])
    with np.errstate(all="ignore"):
        ref = oracle.compute_weights_cart(oracle.OracleMap(maps, mask, 1.0), rows, cols, scan, 0.75, fp, st.copy())
    got = X.weights_cart(oracle, maps, mask, 1.0, rows, cols, scan, 0.75, fp, st)
    assert np.array_equal(_bits(got), _bits(ref))
    assert np.isnan(ref).any() and (ref > 0).sum() > n // 3


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("name", T.NAMES)
def test_b_oracle_within_1e5_of_the_exact_reference_on_every_gpu_case(oracle, name, kind):
    case, exact, ref = T.references(oracle, name, kind)
    assert T.int_form_expected(case["scan"], case["maps"]) == (case["form"] == "integer")
    assert np.array_equal(np.isnan(exact), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(exact[ok] == 0, ref[ok] == 0)
    err = np.abs(exact[ok].astype(np.float64) - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    print(f"{name} {kind}: oracle off the exact reference by {err.max(initial=0.0):.3e}; {int(ok.sum())} of {len(ref)} finite")
    assert err.max(initial=0.0) <= 1e-5
    assert ok.sum() >= len(ref) // 2 and (~ok).any()   # windows inside the map and windows mostly outside it


def test_b_the_limits_the_cases_are_named_for(oracle):
    """The case table reaches what it says: the bounds on both sides of 2^24 and the wrapped one, lists of P entries, a
    dictionary integer just below 2^32 with class sums close to 2^64, and a class total past 2^53 whose float depends on
    rounding once."""
    scans = {n: T.make_case(oracle, n, "polar")["scan"] for n in T.NAMES}
    assert T.mass_bound(scans["mass_bound_2p24_minus_1"]) == 2 ** 24 - 1
    assert T.mass_bound(scans["mass_bound_2p24"]) == 2 ** 24 and scans["mass_bound_2p24"].sum(dtype=np.float64) < 2 ** 32
    assert T.mass_bound(scans["mass_bound_wraps"]) == 2 ** 32
    assert set(T.LADDER) <= set(scans["ladder"].ravel().astype(np.int64).tolist())
    assert ((scans["every_bin_listed"] >= 4096).sum(axis=0) == 2).all()
    several = scans["several_classes"]
    assert ((several > 2 ** 20).sum(axis=0) >= 2).sum() >= 30 and several.sum(axis=0).max() == 2 ** 24 - 4
    for kind in T.KINDS:
        case = T.make_case(oracle, "dictionary_below_2p32", kind)
        q = X.map_power(case["maps"])
        assert q == 23 and 2 ** 32 - 2 ** 10 < float(case["maps"].max()) * 2 ** q < 2 ** 32
        sums = []
        T.exact_weights(oracle, case, sums=sums)
        top = max(max(tot) for tot, _ in sums)
        assert 2 ** 63 < top < 2 ** 64, top.bit_length()
        assert float(T.make_case(oracle, "dictionary_at_2p32", kind)["maps"].max()) * 2 ** 23 == 2 ** 32
        # the made total of particle 0, and weights that differ when the sum goes through a double
        case = T.make_case(oracle, "class_sum_past_2p53", kind)
        cls, made = case["made_total"]
        sums = []
        exact = T.exact_weights(oracle, case, sums=sums)
        assert sums[0][0][cls] == made and 2 ** 53 < made < 2 ** 60
        assert X.round_to_f32(made, 23) != f32(np.ldexp(float(made), -23))
        twice = T.exact_weights(oracle, case, through_double=True)
        assert _bits(exact)[0] != _bits(twice)[0]
        past = sum(1 for tot, _ in sums if 2 ** 53 < max(tot) < 2 ** 60)
        print(f"{kind}: {past} particles with a class total past 2^53, {int((_bits(exact) != _bits(twice)).sum())} weights move")


def test_c_rounding_routine_on_hand_made_ties():
    r = X.round_to_f32
    # 2^24: the first integers a float cannot hold
    assert r(2 ** 24) == f32(2 ** 24) and r(2 ** 24 - 1) == f32(16777215)
    assert r(2 ** 24 + 1) == f32(2 ** 24)          # tie, even below
    assert r(2 ** 24 + 2) == f32(2 ** 24 + 2)
    assert r(2 ** 24 + 3) == f32(2 ** 24 + 4)      # tie, even above
    assert r(2 ** 25 - 1) == f32(2 ** 25)          # tie that carries into the next binade
    # 2^53: the unit of a float there is 2^30
    u = 2 ** 30
    assert r(2 ** 53) == f32(2.0 ** 53)
    assert r(2 ** 53 + u // 2) == f32(2.0 ** 53)                    # tie, even below
    assert r(2 ** 53 + u // 2 + 1) == f32(2.0 ** 53 + u)            # one past the tie
    assert r(2 ** 53 + u + u // 2) == f32(2.0 ** 53 + 2 * u)        # tie, even above
    assert r(2 ** 53 + u + u // 2 - 1) == f32(2.0 ** 53 + u)
    # 2^53 + 2^29 +- 1: where rounding to double first goes wrong (a double's unit is 2 there: the 1 is a tie of its own)
    assert r(2 ** 53 + 2 ** 29 + 1) == f32(2.0 ** 53 + u) and r(2 ** 53 + 2 ** 29 - 1) == f32(2.0 ** 53)
    assert f32(float(2 ** 53 + 2 ** 29 + 1)) == f32(2.0 ** 53)      # (the double rounding under test: down, wrongly)
    assert r(2 ** 53 + 3 * 2 ** 29 - 1) == f32(2.0 ** 53 + u)
    assert f32(float(2 ** 53 + 3 * 2 ** 29 - 1)) == f32(2.0 ** 53 + 2 * u)
    # the power of two only moves the exponent
    assert r(2 ** 53 + 2 ** 29 + 1, 23) == f32((2.0 ** 53 + u) / 2 ** 23) and r(3, 1) == f32(1.5) and r(0, 23) == 0
    assert r(2 ** 64 - 1) == f32(2.0 ** 64)
    # against exact rational comparison on random integers of every size up to 64 bits
    from fractions import Fraction
    rng = np.random.default_rng(3)
    for bits in range(1, 64):
        for _ in range(20):
            n = int(rng.integers(0, 2 ** 63)) >> (63 - bits) | (1 << (bits - 1))
            got = r(n)
            lo, hi = np.nextafter(got, f32(0)), np.nextafter(got, f32(np.inf))
            d = abs(Fraction(float(got)) - n)
            assert d <= abs(Fraction(float(lo)) - n) and d <= abs(Fraction(float(hi)) - n)


def test_c_map_power_and_exact_sums():
    assert X.map_power(np.asarray([[[0.0, 1.0, 50.0]]], f32)) == 0
    assert X.map_power(np.asarray([[[0.0, 1.5, 0.375]]], f32)) == 3
    assert X.map_power(np.asarray([[[np.sqrt(2.0), 50.0]]], f32)) == 23
    assert X.map_power(np.asarray([[[2.0 ** -23, 512 - 2.0 ** -14]]], f32)) == 23
    rng = np.random.default_rng(4)
    c = rng.integers(0, 2 ** 32, 5000, dtype=np.uint64)
    v = rng.integers(0, 2 ** 63, 5000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    assert X.exact_dot(c, v) == sum(int(a) * int(b) for a, b in zip(c, v))
