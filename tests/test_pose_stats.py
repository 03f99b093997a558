"""The pose statistics on the device (tdr_k_mean_cov: one workgroup up to 4096 particles, mc_sums / mc_cov / mc_final above)
against the exact reference of tests/pose_ref.py, at the particle counts where the code changes path and at those the
filter runs at — and the small kernels next to them (tdr_k_sample_ml_states, tdr_k_save_ml_state, tdr_k_set_scale), bit for
bit against their float32 expressions.  Run with `pytest -m gpu`; the reference checks itself in tests/test_pose_ref.py.

Tolerances (derived in tests/pose_ref.py, "ulp" = float32 spacing at the reference value) and the largest deviation seen
on an MI355X over every case below (the 24 floats were the exact reference's bits in every case):

    mean x, y, scale      <= 2 ulp                                          seen: 0 ulp
    mean heading          <= 1e-6 rad                                       seen: 0 rad
    covariance, 16 x      <= 2 ulp + 256 * 2^-53 * sum|term| / (n - 1)      seen: 0 (about the mean and about `about`)
    geometric-mean scale  <= 2 ulp                                          seen: 0 ulp
"""
import math

import numpy as np
import pytest

import pose_ref as P

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = 37


@pytest.fixture(scope="module")
def k():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def _cases():
    return [(n, f) for n in P.SIZES for f in P.FAMILIES if n < P.LARGE or f == "turns"]


def _run(k, ref, cap):
    """tdr_k_mean_cov of ref's particles in [7][cap] planes (NaN behind n): about the mean, and about ref.about."""
    st = k.to_device(P.to_planes(ref.st, cap))
    out = k.mean_cov(st, ref.n)[:24].cpu().numpy()
    out_about = k.mean_cov(st, ref.n, about=k.to_device(ref.about))[:24].cpu().numpy()
    return out, out_about


def _check(ref, out, out_about):
    dev = P.check_means(out, ref)
    # the covariance about the mean: about the mean the device returned, which the line above has just held to the
    # reference — a last-place difference of the mean then stays out of this comparison
    dev["cov"] = P.check_cov(out, ref, out[:4])
    # computeCov: the means do not change, the covariance is about the given point
    assert np.array_equal(out_about[:4].view(np.uint32), out[:4].view(np.uint32))
    assert np.array_equal(out_about[20:24].view(np.uint32), out[20:24].view(np.uint32))
    dev["cov_about"] = P.check_cov(out_about, ref, ref.about)
    return dev


@pytest.mark.parametrize("n,family", _cases())
def test_mean_cov_against_the_exact_reference(k, n, family):
    """Every size at which tdr_k_mean_cov takes another path or a stride ends (1 .. 1025, 4095 / 4096 / 4097, 32 767 /
    32 768 / 32 769, 100 003, 2 000 003), three input families (a converged cluster at the +-pi cut; whole turns added; one
    scale for all), the planes padded with NaN; the two largest sizes run the family with the whole turns only."""
    ref = P.Ref.get(n, family)
    out, out_about = _run(k, ref, n + PAD)
    dev = _check(ref, out, out_about)
    print(f"n = {n}, {family}: deviations (fractions of the tolerances; heading in rad) {dev}")
    if family == "one_scale":
        # a frozen filter frozen again keeps its scale
        assert out[20] == P.ONE_SCALE
    if n == 1:
        x, y, th, sc = P.ml_states(ref.st)
        assert out[0] == x[0] and out[1] == y[0] and out[3] == sc[0]
        turns = round((float(th[0]) - float(out[2])) / (2 * math.pi))
        assert abs(float(th[0]) - 2 * math.pi * turns - float(out[2])) <= P.HEADING_TOL
        assert not np.isfinite(out[4:20]).any() and not np.isfinite(out_about[4:20]).any()
    if n == 2:
        assert np.isfinite(out[:21]).all() and np.isfinite(out_about[:21]).all()


@pytest.mark.parametrize("n", [1025, 4097])
def test_mean_cov_with_no_padding(k, n):
    """cap == n: the planes follow each other without a gap."""
    ref = P.Ref.get(n, "cluster")
    _check(ref, *_run(k, ref, n))


def test_one_particle_gives_its_own_state_and_a_nan_covariance(k, oracle):
    """n = 1 like the reference (it divides by size() - 1 = 0 too): the mean is the particle's mlState, every covariance
    entry NaN — with a heading atan2f(sinf, cosf) returns exactly (0), so that the heading difference is 0 and not a last
    place of it, whose square over 0 would be inf; oracle.mean_cov gives the same."""
    st = P.make_states(1, "cluster")
    st["theta"][0] = 0.0
    out = k.mean_cov(k.to_device(P.to_planes(st, 1 + PAD)), 1)[:24].cpu().numpy()
    x, y, th, sc = P.ml_states(st)
    assert np.array_equal(out[:4], np.array([x[0], y[0], 0.0, sc[0]], F32))
    assert np.isnan(out[4:20]).all()
    assert out[20] == sc[0] and not out[21:24].any()
    om, oc = oracle.mean_cov(st)
    assert np.array_equal(om, out[:4]) and np.isnan(oc).all()


# ---- the small kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,num", [(1, 1), (7, 7), (1000, 1000), (1001, 1000), (100_003, 1000), (3_000_001, 1000)])
def test_sample_ml_states_indices_and_floats(k, n, num):
    """computeGMM's sample: particle min(n - 1, i * n // num) for i < num (i * n passes 2^31 in the last case), its
    mlState().head<3>() in the float32 expressions, bit for bit."""
    st = P.make_states(n, "turns", seed=n + num)
    got = k.sample_ml_states(k.to_device(P.to_planes(st, n + PAD)), n, num).cpu().numpy()
    idx = np.minimum(n - 1, np.arange(num, dtype=np.int64) * n // num)
    assert idx[-1] == (num - 1) * n // num and (n < 3_000_000 or int(idx[-1]) * num > 2 ** 31)
    x, y, th, _ = P.ml_states(st[idx])
    want = np.stack([x, y, th], axis=1)
    assert got.shape == (num, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _ml_record(st, i):
    x, y, th, sc = P.ml_states(st[i:i + 1])
    fields = [st[f][i] for f in P.FIELDS] + [F32(st["have_init"][i])]
    return np.array(fields + [0.0, x[0], y[0], th[0], sc[0]], F32)


def _info(k, word):
    info = np.zeros(8, np.int32)
    info[0] = word
    return k.to_device(info.view(F32))


@pytest.mark.parametrize("n", [1, 15, 4097])
def test_save_ml_state_from_the_planes(k, n):
    """The 12-float record of the particle info[0] names, from [7][cap] planes; an index word out of range selects
    particle 0."""
    st = P.make_states(n, "turns", seed=40 + n)
    dev = k.to_device(P.to_planes(st, n + PAD))
    for word, want in ((n - 1, n - 1), (n // 2, n // 2), (0, 0), (n, 0), (-3, 0), (0x7F800000, 0), (n + PAD - 1, 0)):
        out = k.to_device(np.full(12, np.nan, F32))
        k.save_ml_state(_info(k, word), dev, n, out)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), _ml_record(st, want).view(np.uint32)), (word, want)


@pytest.mark.parametrize("world,shard", [(3, 5), (8, 12_500)])
def test_save_ml_state_from_the_gathered_shards(k, world, shard):
    """The same record from the all-gathered [rank][7][src_shard] buffer, the winner in a rank > 0."""
    n = world * shard
    st = P.make_states(n, "turns", seed=world + shard)
    buf = np.empty((world, 7, shard), F32)
    for r in range(world):
        buf[r] = P.to_planes(st[r * shard:(r + 1) * shard], shard)
    dev = k.to_device(buf)
    for word, want in ((n - 1, n - 1), (shard, shard), (2 * shard + 1, 2 * shard + 1), (shard - 1, shard - 1), (n, 0),
                       (-1, 0)):
        out = k.to_device(np.full(12, np.nan, F32))
        k.save_ml_state(_info(k, word), dev, n, out, src_shard=shard)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), _ml_record(st, want).view(np.uint32)), (word, want)


@pytest.mark.parametrize("n,pad", [(1, PAD), (255, PAD), (256, PAD), (257, PAD), (4097, PAD), (4097, 0)])
def test_set_scale_writes_rows_0_to_n_of_the_scale_plane_only(k, n, pad):
    st = P.make_states(n, "cluster", seed=n + pad)
    before = P.to_planes(st, n + pad)
    dev = k.to_device(before)
    value = F32(1.2345678)
    k.set_scale(dev, n, k.to_device(np.array([value], F32)))
    after = dev.cpu().numpy()
    want = before.copy()
    want[5, :n] = value
    assert np.array_equal(after.view(np.uint32), want.view(np.uint32))


def test_freeze_scale_of_a_filter_above_the_switch(k):
    """freezeScale() of a ParticleFilter of 4097 particles (the multi-workgroup statistics): afterwards every particle's
    scale is the geometric mean the statistics returned, which is the exact reference's to 2 ulp; nothing else moved."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import synth
    sc = synth.make_scene("c1", with_particles=False)
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    ref = P.Ref.get(4097, "cluster")
    f = pkg.ParticleFilter(4097, m, pkg.FilterParams(fixed_scale=-1.0), kernels=k, init_particles=False)
    f.set_states(ref.st.view(pkg.STATE_DTYPE))
    geo = k.mean_cov(f.st, 4097)[20].item()
    assert f.scale() == -1.0
    f.freezeScale()
    assert f.isScaleFrozen()
    got = f.get_states()
    assert np.all(got["scale"] == F32(geo)) and F32(f.scale()) == F32(geo)
    assert abs(geo - float(ref.geo)) <= P.GEO_ULPS * float(P.ulp(ref.geo))
    for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "have_init"):
        assert np.array_equal(got[name], ref.st[name]), name
    # frozen again: nothing changes
    f.freezeScale()
    assert np.all(f.get_states()["scale"] == F32(geo))
