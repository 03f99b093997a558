"""Batched node loop (tdr_batch_render_polar, tdr_batch_pose, csrc/tdr_batch_loop.hip; C++ TopDownRenderCoreBatch; Python
top_down_renderer_amd.batch.LoopBatch): K robots' renders, filter steps and pose statistics at once must leave every robot
bit for bit where its own loop — render, propagate + update, publishPoseEst — leaves it."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
sys.path.insert(0, ROOT)

STEPS = 16
MOTION = (0.3, 0.1, 0.005)
RS_MIN, RS_MAX, TARGET = 0.5, 4.0, 6.5


def _L():
    from top_down_renderer_amd import _lib
    return _lib, _lib.load()


# ---- refusals that need no device -----------------------------------------------------------------------------------------
def test_render_refuses_bad_batches_without_a_device():
    _lib, lib = _L()
    cs = (_lib.BatchCloudC * 2)()
    assert lib.tdr_batch_render_polar(None, 0, cs, C.c_float(0.1), 3, 16, 8, None) == -1
    assert "at least one renderer" in lib.tdr_last_error().decode()
    assert lib.tdr_batch_render_polar(None, 2, cs, C.c_float(0.1), 3, 16, 8, None) == -1
    assert "null renderer array" in lib.tdr_last_error().decode()
    arr = (C.c_void_p * 2)(None, None)
    assert lib.tdr_batch_render_polar(arr, 2, None, C.c_float(0.1), 3, 16, 8, None) == -1
    assert "null cloud array" in lib.tdr_last_error().decode()
    assert lib.tdr_batch_render_polar(arr, 2, cs, C.c_float(0.1), 3, 16, 8, None) == -1
    assert "renderer 0 is null" in lib.tdr_last_error().decode()
    dup = (C.c_void_p * 2)(1234, 1234)   # (never dereferenced: the duplicate is refused first)
    assert lib.tdr_batch_render_polar(dup, 2, cs, C.c_float(0.1), 3, 16, 8, None) == -1
    assert "appears twice" in lib.tdr_last_error().decode()


def test_pose_refuses_bad_batches_without_a_device():
    _lib, lib = _L()
    out = (_lib.PoseStatsC * 3)()
    assert lib.tdr_batch_pose(None, 0, out, None) == -1
    assert "at least one filter" in lib.tdr_last_error().decode()
    assert lib.tdr_batch_pose(None, 3, out, None) == -1
    assert "null filter array" in lib.tdr_last_error().decode()
    arr = (C.c_void_p * 3)(None, None, None)
    assert lib.tdr_batch_pose(arr, 3, None, None) == -1
    assert "null output array" in lib.tdr_last_error().decode()
    assert lib.tdr_batch_pose(arr, 3, out, None) == -1
    assert "filter 0 is null" in lib.tdr_last_error().decode()
    dup = (C.c_void_p * 3)(1234, 5678, 1234)
    assert lib.tdr_batch_pose(dup, 3, out, None) == -1
    assert "appears twice" in lib.tdr_last_error().decode()


def test_get_render_refuses_a_null_renderer():
    _lib, lib = _L()
    assert lib.tdr_renderer_get_render(None, None, None) == -1


def test_core_batch_header_compiles():
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_hdr_"), "hdr.o")
    src = os.path.join(os.path.dirname(exe), "hdr.cpp")
    open(src, "w").write('#include "top_down_render/tdr_compat.h"\n#include "top_down_render/top_down_render_core_batch.h"\n'
                         "int main() { TopDownRenderCoreBatch b; return b.lastBatched(); }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", exe],
                   check=True)


# ---- render ---------------------------------------------------------------------------------------------------------------
def _cloud(rng, n, stride, ioff, ncls):
    pts = np.zeros((n, stride), np.float32)
    if n == 0:
        return pts
    pts[:, 0] = rng.normal(0, 20, n)
    pts[:, 1] = rng.normal(0, 20, n)
    pts[:, 2] = rng.normal(0, 1, n)
    pts[:, ioff] = rng.integers(-2, ncls + 3, n)   # labels outside the LUT too
    if n > 10:
        k = max(1, n // 50)
        pts[rng.integers(0, n, k), 0] = np.nan
        pts[rng.integers(0, n, k), 1] = np.inf
        pts[rng.integers(0, n, k), 0] = -np.inf
        pts[rng.integers(0, n, k), ioff] = np.nan
        o = rng.integers(0, n, k)
        pts[o, 0] = pts[o, 1] = 0.0                  # the origin
        pts[rng.integers(0, n, k), ioff] = 300.0     # beyond the 256-entry LUT
    return pts


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 16])
def test_render_batch_equals_render_polar(k):
    from top_down_renderer_amd import batch
    rng = np.random.default_rng(100 + k)
    ncls, nb, nr, ang_res = 6, 100, 25, float(np.float32(2 * np.pi / 100))
    counts = [0, 1, 100_003]
    layouts = [(4, 3), (8, 5), (8, 4)]
    rs, twins, clouds, res = [], [], [], []
    for i in range(k):
        lut = np.full(256, -1, np.int32)
        lut[: ncls + 1] = rng.permutation(ncls + 1) - (i % 2)   # a LUT of its own per renderer
        rs.append(batch.Renderer(lut))
        twins.append(batch.Renderer(lut))
        stride, ioff = layouts[i % len(layouts)]
        clouds.append((_cloud(rng, counts[i % len(counts)] if k > 1 else 100_003, stride, ioff, ncls), stride, ioff))
        res.append(float(np.float32(0.5 + 0.37 * i)))
    for rep in range(2):   # the second round reuses the staging and the renderers' buffers
        batch.render_batch(rs, clouds, res, ang_res, ncls, nb, nr)
        for t, (pts, stride, ioff), r in zip(twins, clouds, res):
            t.render_polar(pts, stride, ioff, r, ang_res, ncls, nb, nr)
        for i, (a, b) in enumerate(zip(rs, twins)):
            ia, pa = a.get_render()
            ib, pb = b.get_render()
            assert np.array_equal(ia, ib) and np.array_equal(pa, pb), (rep, i)
            if len(clouds[i][0]) > 1000:
                assert ia.sum() > 0
        res = [r * 1.5 for r in res]


# ---- pose statistics ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import batch, synth
    cfg = synth.Config("batchloop", 20000, 6, 100, 25, 700, 1000, seed=93)
    sc = synth.make_scene(cfg)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    return cfg, sc, m


def _params(ncls, fixed_scale=-1.0):
    from top_down_renderer_amd.particle_filter import FilterParams
    return FilterParams(fixed_scale=fixed_scale).to_c(ncls)


@pytest.mark.gpu
def test_pose_batch_equals_mean_cov_and_scale(scene):
    from top_down_renderer_amd import batch, synth
    cfg, sc, m = scene
    ncls = sc.class_maps.shape[0]
    rng = np.random.default_rng(3)
    specs = [(n, -1.0, False) for n in (1, 2, 1023, 4096, 4097, 20000, 131_075)]
    specs += [(5000, -1.0, True), (3000, 1.5, False), (0, -1.0, False)]   # frozen, fixed_scale > 0, empty
    fs, twins = [], []
    for i, (n, fixed, freeze) in enumerate(specs):
        st = synth.make_particles(cfg, sc.lab, sc.pose, rng, n=max(n, 1))[:n]
        st["scale"] = rng.normal(1.0, 0.05, n).astype(np.float32)
        pair = []
        for _ in range(2):
            f = batch.FilterHandle(m, max(n, 1), _params(ncls, fixed), seed=50 + i)
            f.set_states(st)
            if freeze:
                f.freeze_scale()
            pair.append(f)
        fs.append(pair[0])
        twins.append(pair[1])
    mean, cov, scale, n = batch.pose_batch(fs)
    for i, t in enumerate(twins):
        st, cv = t.mean_cov()
        assert n[i] == specs[i][0]
        assert np.array_equal(mean[i], st, equal_nan=True), i
        assert np.array_equal(cov[i], cv, equal_nan=True), i
        assert np.float32(scale[i]).tobytes() == np.float32(t.scale()).tobytes(), i
        # afterwards the filter's own calls return the same values (the cache the batch filled)
        st2, cv2 = fs[i].mean_cov()
        assert np.array_equal(st2, st, equal_nan=True) and np.array_equal(cv2, cv, equal_nan=True), i
        assert np.float32(fs[i].scale()).tobytes() == np.float32(t.scale()).tobytes(), i
    assert scale[7] > 0 and scale[8] == np.float32(1.5) and scale[9] == -1.0
    assert not np.any(mean[9]) and not np.any(cov[9])


# ---- the loop -------------------------------------------------------------------------------------------------------------
def _scenario():
    """tests/test_takestep_loop.py's scenario (the map, the cloud, 3072 particles about the true pose with an unknown scale)
    and three more robots: one above 32 768 particles, one whose first update runs the init search, one of 5000."""
    from top_down_renderer_amd import synth
    sc = synth.make_scene("ref", n_particles=16)
    cfg = sc.cfg

    def states(n, seed, uninit=False):
        rng = np.random.default_rng(seed)
        st = synth.make_particles(cfg, sc.lab, sc.pose, rng, n=n, sigma_px=9.0, sigma_deg=4.0, uniform_frac=0.0)
        st["scale"] = rng.normal(1.0, 0.015, n).astype(np.float32)
        no = int(0.04 * n)
        sel = rng.permutation(n)[:no]
        st["scale"][sel] = 2.5
        st["init_x_px"][sel] += rng.normal(0, 60, no).astype(np.float32)
        st["init_y_px"][sel] += rng.normal(0, 60, no).astype(np.float32)
        if uninit:
            st["have_init"][: n // 7] = 0
        return st

    def cloud(seed):
        if seed is None:
            return sc.pts
        rng = np.random.default_rng(seed)
        keep = rng.random(len(sc.pts)) < 0.9
        p = sc.pts[keep].copy()
        p[:, :2] += rng.normal(0, 0.05, (len(p), 2)).astype(np.float32)
        return p

    robots = [(states(3072, 9), 7, cloud(None)), (states(40_000, 21), 11, cloud(1)), (states(2048, 22, uninit=True), 13, cloud(2)),
              (states(5000, 23), 17, cloud(3))]
    return sc, cfg, robots


def _pcl(p):
    out = np.zeros((len(p), 8), np.float32)
    out[:, :3], out[:, 4] = p[:, :3], p[:, 3]
    return out


@pytest.fixture(scope="module")
def loop_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_batch_loop")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_batch_loop.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip",
                    f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def test_facade_batch_loop_compiles(loop_exe):
    assert os.access(loop_exe, os.X_OK)


def _check_split(stats, step):
    batched, standalone = stats
    assert batched >= 2, (step, stats)       # robots 0 and 3 take the batched path on every step
    assert standalone >= (2 if step == 0 else 1), (step, stats)   # robot 1 (> 32 768) always; robot 2 in its init search
    assert batched + standalone == 4


@pytest.mark.gpu
def test_core_batch_matches_standalone_cores(loop_exe):
    sc, cfg, robots = _scenario()
    d = tempfile.mkdtemp(prefix="tdr_batch_loop_")
    open(os.path.join(d, "meta.txt"), "w").write(
        f"{cfg.ncls} {cfg.map_size} {cfg.map_size} {cfg.nb} {cfg.nr} {len(robots)} {STEPS} {RS_MIN} {RS_MAX} {TARGET} "
        f"{cfg.map_resolution}\n")
    np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), np.float32).tofile(os.path.join(d, "maps.bin"))
    np.ascontiguousarray(sc.class_mask.T, np.uint8).tofile(os.path.join(d, "mask.bin"))
    np.asarray([s for _, s, _ in robots], np.uint32).tofile(os.path.join(d, "seeds.bin"))
    np.tile(np.asarray(MOTION, np.float32), (len(robots), 1)).tofile(os.path.join(d, "motion.bin"))
    for r, (st, _, p) in enumerate(robots):
        st.tofile(os.path.join(d, f"states_{r}.bin"))
        _pcl(p).tofile(os.path.join(d, f"pts_{r}.bin"))
    out = subprocess.run([loop_exe, d], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[STEPS] == "ok", out.stdout
    froze, conv = 0, 0
    for k in range(STEPS):
        tag, step, b, s, fz, cv = lines[k].split()
        assert tag == "step" and int(step) == k
        _check_split((int(b), int(s)), k)
        froze |= int(fz)
        conv = int(cv)
    assert froze & 1 and conv & 1, out.stdout   # robot 0 reaches the freeze and the convergence, as in test_takestep_loop


@pytest.mark.gpu
def test_loop_batch_matches_standalone_loops():
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.top_down_render_core import CoreConfig, TopDownRenderCore
    _lib, lib = _L()
    sc, cfg, robots = _scenario()
    ncls, nb, nr = cfg.ncls, cfg.nb, cfg.nr
    ang_res = float(np.float32(2 * np.pi / nb))
    m = batch.MapHandle(sc.class_maps, sc.class_mask, cfg.map_resolution)
    m.sample_pts_polar(nb, nr, ang_res)
    ccfg = CoreConfig(range_scale_min=RS_MIN, range_scale_max=RS_MAX, target_uncertainty_m=TARGET, theta_bins=nb, range_bins=nr)
    fb, ft, rb, rt, cores, clouds = [], [], [], [], [], []
    for st, seed, p in robots:
        for fl in (fb, ft):
            f = batch.FilterHandle(m, len(st), _params(ncls), seed=seed)
            f.set_states(st)
            fl.append(f)
        rb.append(batch.Renderer(sc.lut))
        rt.append(batch.Renderer(sc.lut))
        cores.append(TopDownRenderCore(ccfg))
        clouds.append((_pcl(p), 8, 4))
    loop = batch.LoopBatch(fb, rb, ccfg, ang_res, ncls, nb, nr)
    priors = [MOTION] * len(robots)

    def twin_step():
        ests = []
        for f, r, c, (pts, stride, ioff) in zip(ft, rt, cores, clouds):
            c.last_res_ = c.current_range_scale_
            res = float(c.current_range_scale_)
            r.render_polar(pts, stride, ioff, res, ang_res, ncls, nb, nr)
            f.propagate(*MOTION)
            f.update(r, res)
            c.filter_ = batch.HandleView(f)
            ests.append(c.publishPoseEst())
            c.filter_ = None
        return ests

    def same(k, eb, et):
        for i in range(len(robots)):
            a, b = eb[i], et[i]
            assert np.array_equal(fb[i].states().view(np.uint8), ft[i].states().view(np.uint8)), (k, i)
            assert a.cov.tobytes() == b.cov.tobytes(), (k, i)
            assert (a.ml_state is None) == (b.ml_state is None) and (a.ml_state is None or a.ml_state.tobytes() == b.ml_state.tobytes())
            assert np.float32(a.scale) == np.float32(b.scale) or (np.isnan(a.scale) and np.isnan(b.scale)), (k, i)
            assert (a.range_scale, a.froze_scale, a.converged) == (b.range_scale, b.froze_scale, b.converged), (k, i)
            assert loop.cores[i].lastRes() == cores[i].lastRes(), (k, i)
            assert loop.cores[i].currentRangeScale() == cores[i].currentRangeScale(), (k, i)

    froze_at, conv_at, res0 = None, None, []
    for k in range(STEPS):
        eb = loop.take_step(clouds, priors)
        _check_split(loop.stats, k)
        et = twin_step()
        same(k, eb, et)
        res0.append(et[0].range_scale)
        if et[0].froze_scale:
            froze_at = k
        if et[0].converged and conv_at is None:
            conv_at = k
    assert froze_at is not None and conv_at is not None and conv_at > froze_at
    assert all(a != b for a, b in zip(res0, res0[1:]))

    # refusals on the device: nothing moves, the next step still matches the twins
    other = batch.MapHandle(sc.class_maps, sc.class_mask, cfg.map_resolution)
    f_other = batch.FilterHandle(other, 16, _params(ncls), seed=5)
    with pytest.raises(_lib.TdrError, match="another map"):
        batch.pose_batch(fb + [f_other])
    with pytest.raises(_lib.TdrError, match="too large"):
        batch.render_batch(rb, clouds, 1.0, ang_res, ncls, 40_000, nr)
    arr = (C.c_void_p * len(rb))(*[r.h for r in rb])
    cs = (_lib.BatchCloudC * len(rb))()
    for i, (pts, stride, ioff) in enumerate(clouds):
        cs[i].pts, cs[i].stride, cs[i].ioff, cs[i].n, cs[i].res = (None if i == 2 else pts.ctypes.data), stride, ioff, len(pts), 1.0
    assert lib.tdr_batch_render_polar(arr, len(rb), cs, C.c_float(ang_res), ncls, nb, nr, None) == -1
    assert "null points" in lib.tdr_last_error().decode()
    same(STEPS, loop.take_step(clouds, priors), twin_step())
