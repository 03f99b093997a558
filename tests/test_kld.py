"""GPU: the KLD-sampling count (csrc/tdr_kld.hip, csrc/tdr_host_kld.cpp; include/tdr.h, "KLD-sampling count") against its
NumPy restatement (tests/kld_ref.py), with ==: the keys, the counts through the launchers, the handle, the batch, the C++
classes (tests/cpp/facade_kld.cpp) and the Python mirror; what is refused; the node loop with kld_every.
Sizes are chosen for where the kernel can go wrong (a lane, a wave less one, a wave, a wave plus one, several workgroups
with a ragged end, more particles than one pass of the grid), not for the workload."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kld_cases as KC
import kld_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32
vp = C.c_void_p
SIZES = [1, 63, 64, 65, 4097, 100003]
PARAM_SETS = [KR.Params(4.0, 1, 0), KR.Params(2.5, 36, 3), KR.Params(0.75, 511, 6)]
FIELDS = ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale")


@pytest.fixture(scope="module")
def K():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def _planes(K, states, cap=None, pad=None):
    """(7, cap) device planes of a structured array; [n, cap) is NaN, or the states of `pad`."""
    n = len(states)
    cap = max(n, 1) if cap is None else cap
    a = np.full((7, cap), np.nan, F32)
    for src, lo in ((states, 0), (pad, n)):
        if src is None or len(src) == 0:
            continue
        for i, name in enumerate(FIELDS):
            a[i, lo:lo + len(src)] = src[name]
        a[6, lo:lo + len(src)] = src["have_init"].astype(F32)
    return K.to_device(a)


def _random_states(n, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros(n, KC.STATE_DTYPE)
    st["init_x_px"] = rng.normal(300, 40, n)
    st["init_y_px"] = rng.normal(-50, 40, n)
    st["dx_m"] = rng.normal(0, 8, n)
    st["dy_m"] = rng.normal(0, 8, n)
    st["theta"] = rng.uniform(-10, 10, n)
    st["scale"] = np.exp(rng.uniform(-0.3, 1.0, n))
    st["have_init"] = rng.random(n) < 0.9
    return st


def _lattice(n, step=1, width=1000):
    """One particle per position bin of 4 px: ix = step * (i % width) - step * width / 2, iy = i / width."""
    i = np.arange(n)
    st = np.zeros(n, KC.STATE_DTYPE)
    st["init_x_px"] = 4.0 * (step * (i % width) - step * (width // 2)) + 1.0     # exact in float32 (< 2^24)
    st["init_y_px"] = 4.0 * (i // width) + 1.0
    st["scale"] = 1.0
    st["have_init"] = 1
    return st


def _distributions(n):
    """name -> (states, params) at the largest size; the tests slice [0, n)."""
    rng = np.random.default_rng(n)
    p = KR.Params(4.0, 36, 6)
    one = np.repeat(KC.state(cx=10.0, cy=-7.0, theta=0.3, scale=1.25), n)
    scales = np.zeros(n, KC.STATE_DTYPE)       # keys that differ only in the scale bin: 8000 of its values, then again
    scales["scale"] = ((np.arange(n) % 8000 + 64 * 100).astype(np.uint32) << np.uint32(17)).view(F32)
    scales["have_init"] = 1
    poses = _random_states(1 + n // 7, 5)
    rep = np.tile(poses, 7)[:n]
    rep = rep[rng.permutation(n)]
    mixed = _random_states(n, 6)
    bad = rng.random(n) < 0.05
    mixed["init_x_px"][bad] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    bad2 = rng.random(n) < 0.05
    mixed["scale"][bad2] = rng.choice([np.nan, np.inf, 0.0, -1.0], int(bad2.sum()))
    mixed["have_init"][rng.random(n) < 0.3] = 0
    return {"one_bin": (one, p), "lattice": (_lattice(n), p), "lattice_1024": (_lattice(n, step=1024), p),
            "scale_only": (scales, p), "repeated_7": (rep, KR.Params(2.5, 36, 3)), "mixed": (mixed, KR.Params(2.5, 36, 3))}


@pytest.fixture(scope="module")
def dists():
    return _distributions(SIZES[-1])


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def test_keys_of_the_hand_worked_particles(K):
    st, want = KC.hand_set()
    got = K.kld_keys(_planes(K, st), len(st), KR.Params(4.0, 36, 3).to_c())
    assert [int(g) for g in got] == [int(KR.NO_KEY) if w is None else w for w in want]
    for T in (1, 36, 511):
        hs = KC.states([dict(theta=th) for th, _ in KC.HEADING[T]])
        got = K.kld_keys(_planes(K, hs), len(hs), KR.Params(4.0, T, 0).to_c())
        assert [(int(g) >> 14) & 0x1FF for g in got] == [b for _, b in KC.HEADING[T]], T
    for b in (0, 1, 6):
        ss = KC.states([dict(scale=s) for s, _ in KC.SCALE[b]])
        got = K.kld_keys(_planes(K, ss), len(ss), KR.Params(4.0, 1, b).to_c())
        assert [int(g) & 0x3FFF for g in got] == [w for _, w in KC.SCALE[b]], b


@pytest.mark.parametrize("pi", range(len(PARAM_SETS)))
def test_keys_of_random_particles_equal_the_restatement(K, pi):
    p = PARAM_SETS[pi]
    for n in (1, 63, 64, 65, 4097):
        st = _random_states(n, 100 + n)
        got = K.kld_keys(_planes(K, st, cap=n + 5), n, p.to_c())
        assert np.array_equal(got, KR.keys(st, p)), (n, p)


# ---- counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_bin", "lattice", "lattice_1024", "scale_only", "repeated_7", "mixed"])
def test_counts_equal_the_restatement(K, dists, name):
    st, p = dists[name]
    planes = _planes(K, st)
    ws = K.kld_workspace(len(st))
    for n in SIZES:
        want = KR.count(st, n, p)
        assert K.kld_count(planes, n, p.to_c(), ws) == want, (name, n)
        if name == "lattice":
            assert want == (n, 0)       # one particle per bin: the table half full
        if name == "one_bin":
            assert want == (1, 0)
    assert K.kld_count(planes, 0, p.to_c(), ws) == (0, 0)


def test_particles_behind_n_are_not_read(K, dists):
    st, p = dists["repeated_7"]
    for n in (63, 64, 65, 4097):
        want = KR.count(st, n, p)
        assert K.kld_count(_planes(K, st[:n], cap=n + 300), n, p.to_c()) == want                 # NaN planes behind n
        sentinels = _lattice(300)                                                                # ... or 300 bins more
        sentinels["init_y_px"] += 5000
        assert KR.count(np.concatenate([st[:n], sentinels]), n + 300, p)[0] == want[0] + 300
        assert K.kld_count(_planes(K, st[:n], cap=n + 300, pad=sentinels), n, p.to_c()) == want


def test_same_words_twice_and_the_table_is_cleared(K, dists):
    st, p = dists["lattice"]
    planes = _planes(K, st)
    ws = K.kld_workspace(len(st))
    first = K.kld_count(planes, 100003, p.to_c(), ws)
    assert K.kld_count(planes, 100003, p.to_c(), ws) == first == (100003, 0)
    # a smaller n on the same table: keys left behind by the large call would be found and not counted
    for n in (4097, 65, 1):
        assert K.kld_count(planes, n, p.to_c(), ws) == (n, 0)
    st2, p2 = dists["mixed"]
    assert K.kld_count(_planes(K, st2), 4097, p2.to_c(), ws) == KR.count(st2, 4097, p2)


def test_job_table_equals_the_single_launches(K, dists):
    p = KR.Params(2.5, 36, 3)
    sets = [dists["repeated_7"][0][:4097], dists["mixed"][0][:65], dists["mixed"][0][:0], dists["lattice"][0][:100003],
            _random_states(63, 3)]
    planes = [_planes(K, s, cap=len(s) + 3) for s in sets]
    got = K.kld_count_jobs(planes, [len(s) for s in sets], p.to_c())
    assert got == [KR.count(s, len(s), p) for s in sets]


def test_launchers_refuse_bad_arguments(K):
    from top_down_renderer_amd._lib import KldParamsC
    import torch
    L = K.lib
    d = K.zeros((7, 8))
    out = K.zeros((2,), dtype=torch.int64)
    ws = K.kld_workspace(8)
    ok = KR.Params().to_c()
    for bad in (KldParamsC(0.0, 36, 3, 0.05, 2.3, 1), KldParamsC(float("nan"), 36, 3, 0.05, 2.3, 1),
                KldParamsC(float("inf"), 36, 3, 0.05, 2.3, 1), KldParamsC(4.0, 0, 3, 0.05, 2.3, 1),
                KldParamsC(4.0, 512, 3, 0.05, 2.3, 1), KldParamsC(4.0, 36, -1, 0.05, 2.3, 1), KldParamsC(4.0, 36, 7, 0.05, 2.3, 1)):
        assert L.tdr_k_kld_count(vp(d.data_ptr()), 8, 8, C.byref(bad), vp(ws.data_ptr()), vp(out.data_ptr()), None) == -1
        assert L.tdr_k_kld_keys(vp(d.data_ptr()), 8, 8, C.byref(bad), vp(ws.data_ptr()), None) == -1
    assert L.tdr_k_kld_count(None, 8, 8, C.byref(ok), vp(ws.data_ptr()), vp(out.data_ptr()), None) == -1
    assert L.tdr_k_kld_count(vp(d.data_ptr()), 8, 9, C.byref(ok), vp(ws.data_ptr()), vp(out.data_ptr()), None) == -1   # n > cap
    assert L.tdr_k_kld_count(vp(d.data_ptr()), 8, 8, None, vp(ws.data_ptr()), vp(out.data_ptr()), None) == -1
    assert L.tdr_k_kld_count_jobs(None, 1, C.byref(ok), None) == -1


# ---- the handle ------------------------------------------------------------------------------------------------------------------
N_H = 4097


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene(synth.Config("kld", 4000, 4, 36, 12, 300, 4096, seed=41, res=2.0))


@pytest.fixture(scope="module")
def facade_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_kld")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_kld.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip",
                    f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def _handle(scene, kind, n_max, seed=5):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    cfg = scene.cfg
    m = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    r = batch.Renderer(scene.lut)
    if kind == "cart":
        m.set_window(24, 20)
        r.render_cart(scene.pts, 4, 3, cfg.res, cfg.ncls, 24, 20)
    else:
        m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
        r.render_polar(scene.pts, 4, 3, cfg.res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    f = batch.FilterHandle(m, n_max, FilterParams(fixed_scale=1.0 if kind == "fixed" else -1.0), seed=seed, cart=kind == "cart")
    return f, r


def _spread_states(scene, n, seed, free_scale):
    from top_down_renderer_amd import synth
    rng = np.random.default_rng(seed)
    st = synth.make_particles(scene.cfg, scene.lab, scene.pose, rng, n=n)
    if free_scale:
        st["scale"] = np.exp(rng.normal(0.0, 0.1, n)).astype(F32)
    return st


def _snapshot(f, n_w=None):
    """Everything the handle lets out.  n_w: the weights the last update computed (its particle count BEFORE the resample),
    where that is less than the count now."""
    n = f.num_particles()
    n_w = n if n_w is None else n_w
    means, covs = f.get_gmm()
    return {"states": f.states().tobytes(), "w": f.weights()[:n_w].tobytes(), "raw": f.raw_weights(n_w).tobytes(),
            "idx": f.resample_indices().tobytes(), "steps": f.step_count(), "gmm": means.tobytes() + covs.tobytes(),
            "n": n, "mean_cov": b"".join(a.tobytes() for a in f.mean_cov())}


@pytest.mark.parametrize("kind", ["polar", "cart", "fixed"])
def test_handle_counts_and_leaves_the_filter_alone(K, scene, kind):
    p = KR.Params(2.5, 36, 3, 0.15, 2.326, 64)
    cfg = scene.cfg
    st = _spread_states(scene, N_H - 100, 7, kind != "fixed")
    pair = [_handle(scene, kind, N_H) for _ in range(2)]      # the twin makes the same calls without the count
    for f, r in pair:
        f.set_states(st)
        f.propagate(0.3, 0.1, 0.005)
        f.update(r, cfg.res, 3001)                              # a resampled set of another size
        f.compute_gmm()
    (f, r), (twin, rt) = pair
    for stage in ("resampled", "propagated"):
        before = _snapshot(f)
        cur = f.states()
        got = f.kld_count(p)
        assert got == KR.target_of(cur, len(cur), p, N_H), (kind, stage)
        assert _snapshot(f) == before == _snapshot(twin), (kind, stage)
        assert got[:2] == K.kld_count(_planes(K, cur, cap=len(cur) + 9), len(cur), p.to_c())     # the launcher
        f.propagate(0.3, 0.1, 0.005)                            # the generator stands where the twin's does
        twin.propagate(0.3, 0.1, 0.005)
        assert f.states().tobytes() == twin.states().tobytes(), (kind, stage)
    assert got[0] > 1 and got[1] == 0
    n_before = f.num_particles()
    f.update(r, cfg.res, got[2])
    twin.update(rt, cfg.res, got[2])
    assert f.num_particles() == got[2] and _snapshot(f, n_before) == _snapshot(twin, n_before)
    # every clamp of the target through the handle
    assert f.kld_count(KR.Params(2.5, 36, 3, 1e-6, 2.326, 64))[2] == N_H                          # the cap
    assert f.kld_count(KR.Params(2.5, 36, 3, 50.0, 0.0, 1))[2] == 3 * f.num_particles() // 4 + 10   # the shrink limit
    assert f.kld_count(KR.Params(2.5, 36, 3, 50.0, 0.0, N_H - 1))[2] == N_H - 1                   # n_min


def test_an_empty_filter_counts_nothing(scene):
    f, _ = _handle(scene, "polar", 500)
    assert f.num_particles() == 0
    assert f.kld_count(KR.Params(n_min=3)) == (0, 0, 10)
    assert f.kld_count(KR.Params(n_min=64)) == (0, 0, 64)
    g, _ = _handle(scene, "polar", 7)
    assert g.kld_count(KR.Params(n_min=64)) == (0, 0, 7)


def test_python_filter_and_cpp_classes_equal_the_handle(K, scene, facade_exe):
    import top_down_renderer_amd as pkg
    p = KR.Params(2.5, 36, 3, 0.15, 2.326, 64)
    cfg = scene.cfg
    n = 4096
    sets = [_spread_states(scene, n, 20 + r, False) for r in range(3)]
    sets[1]["have_init"][::3] = 0
    sets[2]["init_x_px"][::5] = np.nan
    want = [KR.target_of(s, n, p, n) for s in sets]
    # Python ParticleFilter.kldCount on torch buffers
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    pf = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=1, kernels=K, init_particles=False)
    for s, w in zip(sets, want):
        pf.set_states(s)
        assert pf.kldCount(pkg.KldParams(2.5, 36, 3, 0.15, 2.326, 64)) == w[2] and pf.last_kld_ == w[:2]
        assert pf.get_states().tobytes() == s.tobytes()
    # ParticleFilter::kldCount, ParticleFilterBatch::kldCount, ParticleFilterCartesian::kldCount
    d = tempfile.mkdtemp(prefix="tdr_kld_")
    _write_inputs(d, scene, np.concatenate(sets), n, 3, p, steps=0, kld_every=0)
    r = subprocess.run([facade_exe, "count", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.split()[0] in ("polar", "batch", "cart")]
    assert [(w, int(a), int(b)) for w, a, b in lines] == \
        [("polar", w[0], w[2]) for w in want] + [("batch", w[0], w[2]) for w in want] + [("cart", want[0][0], want[0][2])]


# ---- the batch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 16])
def test_batch_equals_the_single_calls(scene, k):
    from top_down_renderer_amd import batch
    p = KR.Params(2.5, 36, 3, 0.15, 2.326, 64)
    sizes = [4097, 0, 65, 100003, 1, 63, 64, 2000, 3000, 5, 640, 64, 1000, 129, 4096, 300][:k] if k > 1 else [4097]
    fs, n_max = [], [max(n, 1) + i for i, n in enumerate(sizes)]
    for i, n in enumerate(sizes):
        f, _ = _handle(scene, "cart" if i == 2 else "polar", n_max[i], seed=30 + i)
        if n:
            st = _spread_states(scene, n, 40 + i, True)
            if i % 4 == 3:
                st["scale"][::7] = np.nan
            f.set_states(st)
        fs.append(f)
    single = [f.kld_count(p) for f in fs]
    states = [f.states() if n else np.zeros(0, KC.STATE_DTYPE) for f, n in zip(fs, sizes)]
    kk, sk, tt = batch.kld_count(fs, p)
    assert list(zip(kk.tolist(), sk.tolist(), tt.tolist())) == single
    for f, n, cur, cap, s in zip(fs, sizes, states, n_max, single):
        assert s == KR.target_of(cur, n, p, cap)
        assert n == 0 or f.states().tobytes() == cur.tobytes()
    kk2, sk2, tt2 = batch.kld_count(fs[::-1], p)       # the staging and the tables are reused: another order, same numbers
    assert list(zip(kk2.tolist(), sk2.tolist(), tt2.tolist())) == single[::-1]


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _bad_params():
    from top_down_renderer_amd._lib import KldParamsC
    nan, inf = float("nan"), float("inf")
    return [KldParamsC(0.0, 36, 3, 0.05, 2.3, 1), KldParamsC(-1.0, 36, 3, 0.05, 2.3, 1), KldParamsC(nan, 36, 3, 0.05, 2.3, 1),
            KldParamsC(inf, 36, 3, 0.05, 2.3, 1), KldParamsC(4.0, 0, 3, 0.05, 2.3, 1), KldParamsC(4.0, 512, 3, 0.05, 2.3, 1),
            KldParamsC(4.0, 36, -1, 0.05, 2.3, 1), KldParamsC(4.0, 36, 7, 0.05, 2.3, 1), KldParamsC(4.0, 36, 3, 0.0, 2.3, 1),
            KldParamsC(4.0, 36, 3, nan, 2.3, 1), KldParamsC(4.0, 36, 3, inf, 2.3, 1), KldParamsC(4.0, 36, 3, 0.05, -0.1, 1),
            KldParamsC(4.0, 36, 3, 0.05, nan, 1), KldParamsC(4.0, 36, 3, 0.05, inf, 1), KldParamsC(4.0, 36, 3, 0.05, 2.3, 0)]


def test_refusals_write_nothing_and_change_nothing(scene):
    from top_down_renderer_amd import batch
    f, r = _handle(scene, "polar", 300)
    g, _ = _handle(scene, "polar", 300, seed=6)
    st = _spread_states(scene, 256, 3, True)
    for h in (f, g):
        h.set_states(st)
    f.propagate(0.1, 0.0, 0.0)
    f.update(r, scene.cfg.res)
    L = f.L
    before = _snapshot(f)
    ok = KR.Params().to_c()
    out = [C.c_int64(777) for _ in range(3)]
    refs = [C.byref(o) for o in out]
    arr2 = (vp * 2)(f.h, g.h)
    o3 = [np.full(2, 777, np.int64) for _ in range(3)]
    p3 = [a.ctypes.data_as(vp) for a in o3]

    def refused(rc, word):
        assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
        assert [o.value for o in out] == [777] * 3 and all((a == 777).all() for a in o3)
        assert _snapshot(f) == before

    refused(L.tdr_filter_kld_count(None, C.byref(ok), *refs), "null")
    refused(L.tdr_filter_kld_count(f.h, None, *refs), "null")
    for bad in _bad_params():
        refused(L.tdr_filter_kld_count(f.h, C.byref(bad), *refs), "kld_count")
        refused(L.tdr_batch_kld_count(arr2, 2, C.byref(bad), *p3, None), "kld_count")
    refused(L.tdr_batch_kld_count(None, 2, C.byref(ok), *p3, None), "null")
    refused(L.tdr_batch_kld_count(arr2, 0, C.byref(ok), *p3, None), "at least one")
    refused(L.tdr_batch_kld_count(arr2, 2, None, *p3, None), "null")
    refused(L.tdr_batch_kld_count((vp * 2)(f.h, None), 2, C.byref(ok), *p3, None), "null")
    refused(L.tdr_batch_kld_count((vp * 2)(f.h, f.h), 2, C.byref(ok), *p3, None), "twice")
    # outputs are optional
    assert L.tdr_filter_kld_count(f.h, C.byref(ok), None, None, None) == 0
    assert L.tdr_batch_kld_count(arr2, 2, C.byref(ok), None, None, p3[2], None) == 0 and (o3[2] != 777).all()
    assert _snapshot(f) == before
    with pytest.raises(ValueError):
        from top_down_renderer_amd.particle_filter import KldParams, kld_params_c
        kld_params_c(KldParams(epsilon=0.0))


def test_a_sharded_filter_is_refused(scene):
    """One rank over the callback transport: the collectives are copies on the device."""
    from top_down_renderer_amd import FilterParams
    from top_down_renderer_amd._lib import check
    f, _ = _handle(scene, "polar", 64)
    L = f.L
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    AG = C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_size_t, vp)
    BC = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, vp)

    class Ops(C.Structure):
        _fields_ = [("ctx", vp), ("all_gather", AG), ("broadcast", BC)]
    ops = Ops(None, AG(lambda ctx, send, recv, nbytes, stream: hip.hipMemcpy(recv, send, nbytes, 3)),
              BC(lambda ctx, buf, nbytes, root, stream: 0))
    comm, sh = vp(), vp()
    check(L.tdr_comm_create(1, 0, C.byref(ops), C.byref(comm)))
    fp = FilterParams(fixed_scale=1.0).to_c(scene.cfg.ncls)
    check(L.tdr_filter_create_sharded(f.map.h, 64, C.byref(fp), 7, comm, C.byref(sh)))
    try:
        ok = KR.Params().to_c()
        out = [C.c_int64(777) for _ in range(3)]
        assert L.tdr_filter_kld_count(sh, C.byref(ok), *[C.byref(o) for o in out]) == -1
        assert "sharded" in L.tdr_last_error().decode() and [o.value for o in out] == [777] * 3
        o3 = [np.full(2, 777, np.int64) for _ in range(3)]
        assert L.tdr_batch_kld_count((vp * 2)(f.h, sh), 2, C.byref(ok), *[a.ctypes.data_as(vp) for a in o3], None) == -1
        assert "sharded" in L.tdr_last_error().decode() and all((a == 777).all() for a in o3)
    finally:
        L.tdr_filter_destroy(sh)
        L.tdr_comm_destroy(comm)
    # the Python filter with an active group raises before it touches the device
    import types
    from top_down_renderer_amd import KldParams, ParticleFilter
    pf = ParticleFilter.__new__(ParticleFilter)
    pf.comm = types.SimpleNamespace(active=True)
    with pytest.raises(ValueError, match="sharded"):
        pf.kldCount(KldParams())


# ---- the node loop ---------------------------------------------------------------------------------------------------------------
STEPS = 12
MOTION = (0.3, 0.1, 0.005)
LOOP_P = KR.Params(4.0, 36, 3, 0.15, 2.326, 64)


def _write_inputs(d, sc, states, npart, robots, p, steps, kld_every, gmm_every=0, seed=7):
    cfg = sc.cfg
    open(os.path.join(d, "meta.txt"), "w").write(
        f"{cfg.ncls} {cfg.map_size} {cfg.map_size} {cfg.nb} {cfg.nr} {len(sc.pts)} {npart} {seed} {steps} 1.0 "
        f"{cfg.map_resolution} {kld_every} {gmm_every} {robots} {p.bin_xy_px} {p.theta_bins} {p.scale_bits} {p.epsilon} {p.z} "
        f"{p.n_min}\n")
    np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), F32).tofile(os.path.join(d, "maps.bin"))
    np.ascontiguousarray(sc.class_mask.T, np.uint8).tofile(os.path.join(d, "mask.bin"))
    pcl = np.zeros((len(sc.pts), 8), F32)
    pcl[:, :3], pcl[:, 4] = sc.pts[:, :3], sc.pts[:, 3]
    pcl.tofile(os.path.join(d, "pts.bin"))
    np.ascontiguousarray(states, KC.STATE_DTYPE).tofile(os.path.join(d, "states.bin"))
    np.asarray(MOTION, F32).tofile(os.path.join(d, "motion.bin"))


def _check_trace(trace, n0, every, n_max, p):
    """trace: per step (numParticles, the target in force afterwards or -1, the states).  The count of every step is the
    target the step before left; a due step leaves the restatement's target of its own particle set."""
    n_prev, next_prev = n0, -1
    for s, (n, nxt, st) in enumerate(trace):
        assert n == (next_prev if next_prev >= 0 else n_prev) and len(st) == n, s
        if (s + 1) % every == 0:
            assert nxt == KR.target_of(st, n, p, n_max)[2], s
        else:
            assert nxt == next_prev, s
        n_prev, next_prev = n, nxt
    return [n for n, _, _ in trace]


def _read_trace(d, r, steps):
    counts = np.fromfile(os.path.join(d, f"out_counts_{r}.bin"), np.int64).reshape(steps, 2)
    st = np.fromfile(os.path.join(d, f"out_states_{r}.bin"), KC.STATE_DTYPE)
    assert len(st) == counts[:, 0].sum()
    offs = np.concatenate([[0], np.cumsum(counts[:, 0])])
    return [(int(counts[s, 0]), int(counts[s, 1]), st[offs[s]:offs[s + 1]]) for s in range(steps)]


def test_cpp_core_resamples_to_the_count_of_the_last_step(scene, facade_exe):
    n = 4096
    d = tempfile.mkdtemp(prefix="tdr_kld_")
    _write_inputs(d, scene, scene.states, n, 1, LOOP_P, STEPS, 1)
    r = subprocess.run([facade_exe, "loop", d], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ns = _check_trace(_read_trace(d, 0, STEPS), n, 1, n, LOOP_P)
    assert ns[0] == n and ns[-1] < ns[0], ns            # the cloud condensed


def test_cpp_batch_core_equals_three_single_cores(scene, facade_exe):
    n, robots = 4096, 3
    sets = np.concatenate([_spread_states(scene, n, 60 + r, False) for r in range(robots)])
    traces = {}
    for mode in ("loop", "batch"):
        d = tempfile.mkdtemp(prefix="tdr_kld_")
        _write_inputs(d, scene, sets, n, robots, LOOP_P, STEPS, 2)
        r = subprocess.run([facade_exe, mode, d], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        traces[mode] = [_read_trace(d, i, STEPS) for i in range(robots)]
    for i in range(robots):
        ns = _check_trace(traces["batch"][i], n, 2, n, LOOP_P)
        assert ns[-1] < n
        for (na, ta, sa), (nb, tb, sb) in zip(traces["loop"][i], traces["batch"][i]):
            assert (na, ta) == (nb, tb) and sa.tobytes() == sb.tobytes(), i


def test_two_rules_for_one_number_are_refused(scene, facade_exe):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.top_down_render_core import CoreConfig, TopDownRenderCore
    d = tempfile.mkdtemp(prefix="tdr_kld_")
    _write_inputs(d, scene, scene.states, 4096, 1, LOOP_P, 1, 1, gmm_every=1)
    r = subprocess.run([facade_exe, "loop", d], capture_output=True, text=True)
    assert r.returncode == 3 and "two rules" in r.stderr, r.stderr
    both = CoreConfig(kld_every=1, gmm_every=2)
    with pytest.raises(ValueError, match="two rules"):
        TopDownRenderCore(both).initialize(None, None, None)
    with pytest.raises(ValueError, match="two rules"):
        batch.LoopBatch([None], [None], both, 0.1, 4, 36, 12)


def _loop_cfg(scene, every, n):
    import top_down_renderer_amd as pkg
    cfg = scene.cfg
    return pkg.CoreConfig(particle_count=n, theta_bins=cfg.nb, range_bins=cfg.nr, seed=7, kld_every=every,
                          kld=pkg.KldParams(LOOP_P.bin_xy_px, LOOP_P.theta_bins, LOOP_P.scale_bits, LOOP_P.epsilon, LOOP_P.z,
                                            LOOP_P.n_min))


def test_python_core_resamples_to_the_count_of_the_last_step(K, scene):
    import top_down_renderer_amd as pkg
    cfg, n = scene.cfg, 4096
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
    core = pkg.TopDownRenderCore(_loop_cfg(scene, 1, n), kernels=K)
    core.initialize(m, pkg.FilterParams(fixed_scale=1.0), scene.lut, init_particles=False)
    core.filter_.set_states(scene.states)
    trace = []
    for s in range(STEPS):
        assert core.takeStep(scene.pts, MOTION[:2], MOTION[2]) is not None
        trace.append((core.filter_.numParticles(), -1 if core.kld_target_ is None else core.kld_target_, core.filter_.get_states()))
    ns = _check_trace(trace, n, 1, n, LOOP_P)
    assert ns[0] == n and ns[-1] < ns[0], ns


def test_python_loop_batch_equals_three_single_loops(scene):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    cfg, n, robots = scene.cfg, 4096, 3
    ang = float(cfg.ang_res)
    m = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    m.sample_pts_polar(cfg.nb, cfg.nr, ang)
    pcl = np.zeros((len(scene.pts), 8), F32)
    pcl[:, :3], pcl[:, 4] = scene.pts[:, :3], scene.pts[:, 3]

    def make():
        fs = []
        for r in range(robots):
            f = batch.FilterHandle(m, n, FilterParams(fixed_scale=1.0), seed=70 + r)
            f.set_states(_spread_states(scene, n, 60 + r, False))
            fs.append(f)
        return fs

    fb, fsingle = make(), make()
    loop = batch.LoopBatch(fb, [batch.Renderer(scene.lut) for _ in range(robots)], _loop_cfg(scene, 2, n), ang, cfg.ncls, cfg.nb, cfg.nr)
    singles = [batch.LoopBatch([f], [batch.Renderer(scene.lut)], _loop_cfg(scene, 2, n), ang, cfg.ncls, cfg.nb, cfg.nr)
               for f in fsingle]
    traces = [[] for _ in range(robots)]
    for s in range(STEPS):
        loop.take_step([(pcl, 8, 4)] * robots, [MOTION] * robots)
        for r in range(robots):
            singles[r].take_step([(pcl, 8, 4)], [MOTION])
            c = loop.cores[r]
            assert fb[r].states().tobytes() == fsingle[r].states().tobytes(), (s, r)
            assert c.kld_target_ == singles[r].cores[0].kld_target_
            traces[r].append((fb[r].num_particles(), -1 if c.kld_target_ is None else c.kld_target_, fb[r].states()))
    for r in range(robots):
        assert _check_trace(traces[r], n, 2, n, LOOP_P)[-1] < n
