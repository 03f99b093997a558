"""The high-precision reference of the pose statistics (tests/pose_ref.py) checked on the CPU, before tests/test_pose_stats.py
holds the kernels to it: against the CPU oracle where the oracle's serial float sums are still accurate, against a
hand-worked vector, and against a NumPy emulation of the kernels' own order of float64 additions on the very inputs the
GPU tests use — the reference alone stays inside the tolerances.  The sentinel particles of those inputs are checked here
too: losing any one of them moves an asserted output by at least 64 times its tolerance."""
import math

import numpy as np
import pytest

import pose_ref as P

F32 = np.float32


def _cases():
    return [(n, f) for n in P.SIZES for f in P.FAMILIES if n < P.LARGE or f == "turns"]


@pytest.mark.parametrize("n", [2, 3, 17, 64])
@pytest.mark.parametrize("family", ["cluster", "turns"])
def test_small_sets_agree_with_the_oracle(oracle, n, family):
    """Up to 64 particles the oracle's serial float32 chains are accurate: mean, covariance about the mean and about a far
    point, and the geometric-mean scale agree to 1e-5 relative (cancelling covariance entries: relative to the sum of
    their terms' magnitudes, which is what bounds a float chain's error)."""
    st = P.make_states(n, family, seed=7 * n + len(family))
    om, oc = oracle.mean_cov(st)
    mean, geo, _ = P.mean_ref(st)
    for k in (0, 1, 3):
        assert abs(float(mean[k]) - float(om[k])) <= 1e-5 * abs(float(om[k]))
    assert abs(float(mean[2]) - float(om[2])) <= 1e-5 * math.pi
    assert abs(float(geo) - oracle.freeze_scale(st.copy())) <= 1e-5 * float(geo)      # (the oracle's sets the scales)
    about = P.far_about(st)
    for ref_pt, want in ((om, oc), (about, oracle.cov_about(st, about))):
        cov, absum, _ = P.cov_ref(st, ref_pt)
        bound = 1e-5 * np.maximum(np.abs(want), absum / (n - 1))
        assert np.all(np.abs(cov.astype(np.float64) - want) <= bound), (cov, want)


def test_one_particle_like_the_oracle(oracle):
    """n = 1: the mean is the particle's own mlState, heading wrapped; the covariance divides by size() - 1 = 0."""
    st = P.make_states(1, "turns")
    st["theta"][0] = F32(3.0 + 4 * math.pi)
    om, oc = oracle.mean_cov(st)
    mean, _, _ = P.mean_ref(st)
    x, y, th, sc = P.ml_states(st)
    assert mean[0] == x[0] and mean[1] == y[0] and mean[3] == sc[0]
    assert abs(float(mean[2]) - 3.0) < 2e-6 and abs(float(om[2]) - float(mean[2])) < 1e-6
    cov, _, _ = P.cov_ref(st, om)
    assert not np.isfinite(cov).any() and not np.isfinite(oc).any()
    assert np.array_equal(np.isnan(cov), np.isnan(oc))


def test_hand_worked_three_particles_one_wraps():
    st = np.zeros(3, P.STATE_DTYPE)
    #                 init_x init_y dx   dy   theta scale          x   y
    rows = [(10.0, 20.0, 2.0, 4.0, 3.0, 0.5),                   # 11, 22
            (12.0, 18.0, 1.0, 2.0, -3.0, 2.0),                  # 14, 22
            (5.0, 26.0, 4.0, -1.0, 3.0, 2.0)]                   # 13, 24
    for i, r in enumerate(rows):
        for f, v in zip(P.FIELDS, r):
            st[f][i] = v
    mean, geo, tot = P.mean_ref(st)
    assert tot[0] == 38.0 and tot[1] == 68.0 and tot[3] == 4.5
    assert mean[0] == F32(38.0) / F32(3.0) and mean[1] == F32(68.0) / F32(3.0) and mean[3] == F32(1.5)
    # sin: sin 3 - sin 3 + sin 3, cos: 3 cos 3
    assert abs(float(mean[2]) - math.atan2(math.sin(3.0) / 3, math.cos(3.0))) < 3e-7
    assert abs(float(geo) - 2.0 ** (1.0 / 3.0)) <= float(np.spacing(F32(1.26)))
    # about (12, 22, 3, 1): d = (-1, 0, 0, -.5), (2, 0, w, 1), (1, 2, 0, 1) with w = f32(-6 + 2 pi): particle 1 wraps once
    w = F32(-6.0 + 2 * math.pi)
    cov, absum, _ = P.cov_ref(st, [12.0, 22.0, 3.0, 1.0])
    want = np.array([[3.0, 1.0, w, 1.75],
                     [1.0, 2.0, 0.0, 1.0],
                     [w, 0.0, F32(w * w) / F32(2), w / F32(2)],
                     [1.75, 1.0, w / F32(2), 1.125]], F32)
    assert np.array_equal(cov, want), (cov, want)
    assert absum[0, 0] == 6.0 and absum[0, 3] == 3.5 and absum[1, 2] == 0.0


def test_wrap_runs_as_often_as_it_must():
    d = np.array([math.pi, -math.pi, 3.2, -3.2, 20.0, -20.0, 0.0], F32)
    got = P.wrap(d)
    # f32(pi) is above the double pi: it goes one turn down, to just inside -pi; f32(-pi) the mirror
    assert got[0] == F32(float(d[0]) - 2 * math.pi) and got[0] < 0 and got[1] == -got[0] and got[6] == 0
    assert np.all(np.abs(got.astype(np.float64)) <= math.pi + 1e-6)
    assert abs(float(got[4]) - (20.0 - 6 * math.pi)) < 2e-6 and abs(float(got[5]) + (20.0 - 6 * math.pi)) < 2e-6


@pytest.mark.parametrize("n,family", _cases())
def test_the_kernels_order_of_additions_stays_inside_the_tolerances(n, family):
    """The 24 floats a float64 sum in the kernels' order gives (strided per-thread serial sums, 64-lane shuffle tree, waves
    in order, workgroups in order), held to the exact reference by the assertions of the GPU tests, on their inputs."""
    ref = P.Ref.get(n, family)
    out = P.kernel_order(ref.st)
    dev = P.check_means(out, ref)
    dev["cov"] = P.check_cov(out, ref, out[:4])
    dev["cov_about"] = P.check_cov(P.kernel_order(ref.st, ref.about), ref, ref.about)
    print(f"n = {n}, {family}: deviations (fractions of the tolerances; heading in rad) {dev}")


@pytest.mark.parametrize("n,family", _cases())
def test_losing_any_one_sentinel_particle_shows(n, family):
    """The inputs' own property: without the terms of any ONE sentinel particle (indices 0, n - 1, 4095, 4096, 32 767,
    32 768 where n has them) at least one asserted output is 64 tolerances and more away from the reference."""
    ref = P.Ref.get(n, family)
    idx = P.sentinels(n)
    assert idx and idx[0] == 0 and idx[-1] == n - 1
    for i in idx:
        assert P.sentinel_effect(ref, i) >= 64.0, (n, family, i)


def test_input_families_are_what_they_claim():
    st = P.make_states(4097, "turns")
    assert float(np.abs(st["theta"]).max()) <= 64.0
    d = P.wrap((st["theta"] - F32(3.1)).astype(F32))
    assert np.count_nonzero(np.abs(st["theta"] - F32(3.1)) > 2 * math.pi) > 2000        # several turns of the loop
    assert float(np.abs(d).max()) < 1.0
    one = P.make_states(4097, "one_scale")
    assert np.all(one["scale"] == P.ONE_SCALE)
    _, geo, _ = P.mean_ref(one)
    assert geo == P.ONE_SCALE                                  # exp(log s) in double is within 2^-51 of the float s
    c = P.make_states(4097, "cluster")
    m, _, _ = P.mean_ref(c)
    assert np.count_nonzero(P.wrap((c["theta"] - m[2]).astype(F32)) != (c["theta"] - m[2]).astype(F32)) > 100
    assert abs(float(P.far_about(c)[2]) - float(m[2])) > 3 * 2 * math.pi
    pl = P.to_planes(c, 4097 + 37)
    assert np.isnan(pl[:, 4097:]).all() and not np.isnan(pl[:, :4097]).any()


def test_float_chain_drift_is_why_the_kernels_sum_in_double():
    """The reference's serial float32 sums on a converged cluster of a million particles are pixels off in the mean and a
    multiple off in the covariance (the drift table of DESIGN.md, computed on the CPU): no reference for the kernels there."""
    st = P.make_states(1_000_000, "cluster", seed=5)
    dx, c00, c33 = P.float_chain_drift(st)
    print(f"n = 1 000 000: mean x off by {dx:.3g} px, cov(0,0) by a factor of {1 + c00:.3g}, cov(3,3) by {c33:.2e} relative")
    assert dx > 1.0 and c00 > 1.0
