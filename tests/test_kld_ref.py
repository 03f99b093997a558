"""CPU: the NumPy restatement of the KLD-sampling count (tests/kld_ref.py) against facts worked out by hand
(tests/kld_cases.py and the comments below), and the library's two host functions against the restatement."""
import ctypes as C

import numpy as np
import pytest

import kld_cases as KC
import kld_ref as KR

F32 = np.float32


def _bins(key):
    key = int(key)
    return (key >> 43) - 524288, ((key >> 23) & 0xFFFFF) - 524288, (key >> 14) & 0x1FF, key & 0x3FFF


def test_position_bins_floor_edges_and_clamp():
    p = KR.Params(bin_xy_px=4.0, theta_bins=1, scale_bits=0)
    for c, b in KC.POS_BIN4:
        kx, ky = KR.keys(KC.states([dict(cx=c), dict(cy=c)]), p)
        assert _bins(kx)[:2] == (b, 0), c
        assert _bins(ky)[:2] == (0, b), c
    for kw, want in KC.POS_PRODUCT:
        assert _bins(KR.keys(KC.state(**kw), p)[0])[:2] == want
    # half-pixel bins: 1.25 / 0.5 = 2.5 -> bin 2; -1.25 / 0.5 = -2.5 -> bin -3
    kk = KR.keys(KC.states([dict(cx=1.25, cy=-1.25)]), KR.Params(bin_xy_px=0.5, theta_bins=1, scale_bits=0))
    assert _bins(kk[0])[:2] == (2, -3)


@pytest.mark.parametrize("T", [1, 36, 511])
def test_heading_bins(T):
    p = KR.Params(theta_bins=T)
    for th, b in KC.HEADING[T]:
        assert _bins(KR.keys(KC.state(theta=th), p)[0])[2] == b, th
    # a particle without a heading: bin T, whatever its theta holds, and so a bin of its own at its position
    for th in (0.0, 1.0, -7.3):
        assert _bins(KR.keys(KC.state(theta=th, have_init=0), p)[0])[2] == T
    two = KC.states([dict(theta=0.0), dict(theta=0.0, have_init=0)])
    assert KR.count(two, 2, p) == (2, 0)


@pytest.mark.parametrize("b", [0, 1, 6])
def test_scale_bins(b):
    p = KR.Params(scale_bits=b)
    for s, want in KC.SCALE[b]:
        assert _bins(KR.keys(KC.state(scale=s), p)[0])[3] == want, s


def test_particles_without_a_key_are_skipped_not_counted():
    p = KR.Params()
    st = KC.states(KC.NO_KEY_ROWS)
    assert (KR.keys(st, p) == KR.NO_KEY).all()
    assert KR.count(st, len(st), p) == (0, len(st))
    mixed = np.concatenate([st, KC.states([dict(cx=1.0), dict(cx=2.0), dict(cx=100.0)])])   # bins 0, 0, 25
    assert KR.count(mixed, len(mixed), p) == (2, len(st))
    assert KR.count(mixed, len(st) + 2, p) == (1, len(st))     # only [0, n) is read
    assert KR.count(mixed, 0, p) == (0, 0)


def test_hand_set_keys_bit_for_bit():
    st, want = KC.hand_set()
    got = KR.keys(st, KR.Params(bin_xy_px=4.0, theta_bins=36, scale_bits=3))
    assert len(got) == len(want) > 40
    for g, w in zip(got, want):
        assert int(g) == (int(KR.NO_KEY) if w is None else w)
    assert all(w is None or w < (1 << 63) for w in want)      # bit 63 is clear: the all-ones word is no key


def test_bound_by_hand():
    """epsilon = 0.05, z = 2.326, so (k - 1) / (2 epsilon) = 10 (k - 1).
      k = 2:   a = 2/9 = 0.222222, sqrt a = 0.471405, t = 1 - 0.222222 + 0.471405 * 2.326 = 1.874265, t^3 = 6.58404,
               10 * 6.58404 = 65.84 -> 66
      k = 10:  a = 2/81 = 0.0246914, sqrt a = 0.157135, t = 0.975309 + 0.365496 = 1.340804, t^3 = 2.410439,
               90 * 2.410439 = 216.94 -> 217
      k = 101: a = 2/900 = 0.00222222, sqrt a = 0.0471405, t = 0.997778 + 0.109649 = 1.107426, t^3 = 1.358140,
               1000 * 1.358140 = 1358.14 -> 1359"""
    assert [KR.bound(k, 0.05, 2.326) for k in (0, 1, 2, 10, 101)] == [0, 0, 66, 217, 1359]
    assert KR.bound(2, 0.05, 0.0) == 5        # z = 0: t = 7/9, t^3 = 0.470508, 10 * 0.470508 = 4.7 -> 5
    assert KR.bound(1 << 40, 1e-9, 2.326) == 1 << 62     # 2^40 / 2e-9 = 5.5e20 > 2^62: saturated


def test_target_at_each_clamp():
    assert KR.target(5000, 1000, 100, 10000) == 5000     # the bound itself
    assert KR.target(0, 40, 100, 10000) == 100           # n_min (3 * 40 / 4 + 10 = 40)
    assert KR.target(50, 1000, 100, 10000) == 760        # the shrink limit 3 * 1000 / 4 + 10
    assert KR.target(50, 1001, 100, 10000) == 760        # ... in integers: 3003 / 4 = 750
    assert KR.target(50000, 1000, 100, 10000) == 10000   # the cap
    assert KR.target(0, 0, 1, 5) == 5                    # an empty filter: min(max(n_min, 10), n_max)
    assert KR.target(0, 0, 1, 500) == 10


@pytest.fixture(scope="module")
def lib():
    from top_down_renderer_amd import _lib, build
    build.build()
    return _lib.load()


def test_host_functions_equal_the_restatement(lib):
    ks = list(range(0, 70)) + [100, 101, 999, 4096, 65537, 10 ** 6, 10 ** 9, (1 << 31) + 1, 1 << 40]
    for eps, z in ((0.05, 2.326), (0.01, 0.0), (0.2, 3.0), (1e-9, 2.326)):
        for k in ks:
            assert lib.tdr_kld_bound_host(k, C.c_double(eps), C.c_double(z)) == KR.bound(k, eps, z), (k, eps, z)
    assert lib.tdr_kld_bound_host(1 << 40, C.c_double(1e-9), C.c_double(2.326)) == 1 << 62
    assert lib.tdr_kld_bound_host(-5, C.c_double(0.05), C.c_double(2.326)) == 0
    for n_kld in (0, 1, 66, 760, 761, 5000, 1 << 62):
        for last in (0, 1, 40, 1000, 1001, 250000):
            for n_min in (1, 100, 5000):
                for cap in (5, 4096, 250000):
                    assert lib.tdr_kld_target_host(n_kld, last, n_min, cap) == KR.target(n_kld, last, n_min, cap)


def test_workspace_is_a_power_of_two_of_at_least_two_n_words(lib):
    for n in (0, 1, 31, 32, 33, 4097, 100003, 2000000):
        slots = lib.tdr_kld_workspace_bytes(n) // 8
        assert lib.tdr_kld_workspace_bytes(n) % 8 == 0 and slots >= max(2 * n, 1) and slots & (slots - 1) == 0
        assert slots < max(4 * n, 65)
    assert lib.tdr_kld_workspace_bytes(-1) == 0


def test_params_struct_layout():
    from top_down_renderer_amd import _lib
    assert C.sizeof(_lib.KldParamsC) == 40 and _lib.KldParamsC.epsilon.offset == 16 and _lib.KldParamsC.n_min.offset == 32
    assert C.sizeof(_lib.KldJobC) == 48
