"""GPU: sensor resetting (include/tdr.h, "sensor resetting") through the facades: the Python filter on torch buffers, the C++
classes (tests/cpp/facade_sensor_reset.cpp) and the handle leave the same states; the Python core, the C++ core and a loop
of handle calls agree with recovery_candidates = 8; recovery_candidates = 1 is the loop without the field; a batch that
holds a core with more candidates is refused."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import recovery_ref as RR
from test_recovery import LOOP_RP, MOTION, _handle, _loop_cfg, _python_core_trace, _read_loop, _spread_states, _write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene(synth.Config("recovery", 4000, 4, 36, 12, 300, 4096, seed=41, res=2.0))


def _build(name):
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", PKG, "-ltdr_hip", f"-Wl,-rpath,{PKG}"], check=True)
    return exe


@pytest.fixture(scope="module")
def facade_exe():
    return _build("facade_sensor_reset")


@pytest.mark.parametrize("mode", [0, 1])
def test_python_filter_cpp_classes_and_handle_leave_the_same_states(K, scene, facade_exe, mode):
    import top_down_renderer_amd as pkg
    cfg, n, p, seed, C_ = scene.cfg, 2048, 0.02, 900, 8
    sets = [_spread_states(scene, n, 20 + r, False) for r in range(2)]
    # the handle: polar filters on the two sets, a Cartesian one on the first
    want = []
    for r, s in enumerate(sets):
        f, rend = _handle(scene, "fixed", n, seed=7 + r)
        f.set_states(s)
        cnt = f.inject_sensor(rend, cfg.res, p, C_, mode, seed + r)
        want.append((f.states(), cnt))
        assert 20 < cnt < 70
    from top_down_renderer_amd import batch
    mc = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    mc.set_window(cfg.nb, cfg.nr)                                       # the window the C++ program sets
    rc = batch.Renderer(scene.lut)
    rc.render_cart(scene.pts, 4, 3, cfg.res, cfg.ncls, cfg.nb, cfg.nr)
    fc = batch.FilterHandle(mc, n, pkg.FilterParams(fixed_scale=1.0), seed=7, cart=True)
    fc.set_states(sets[0])
    want_cart = (fc.inject_sensor(rc, cfg.res, p, C_, mode, seed), fc.states())
    # the Python filter on torch buffers
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    rp = pkg.ScanRendererPolar(scene.lut, kernels=K)
    rp.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    rp.renderSemanticTopDown(scene.pts, cfg.res, cfg.ang_res)
    pf = pkg.ParticleFilter(n, m, pkg.FilterParams(fixed_scale=1.0), seed=1, kernels=K, init_particles=False)
    for r, (s, (w, cnt)) in enumerate(zip(sets, want)):
        pf.set_states(s)
        assert pf.injectSensor(rp.last_scan(), cfg.res, p, C_, mode, seed + r) == cnt
        assert pf.get_states().tobytes() == w.tobytes(), (mode, r)
        assert pf._maybe_uninit == (mode == 0)
    for bad in (dict(p=1.5), dict(candidates=0), dict(candidates=4097), dict(heading_mode=2), dict(res=0.0), dict(res=float("nan"))):
        kw = dict(dict(top_down_scan=rp.last_scan(), res=cfg.res, p=p, candidates=C_, heading_mode=mode), **bad)
        with pytest.raises(ValueError):
            pf.injectSensor(**kw)
    assert pf.get_states().tobytes() == want[-1][0].tobytes()
    # ParticleFilter::injectSensor, ParticleFilterCartesian::injectSensor
    d = tempfile.mkdtemp(prefix="tdr_sensor_")
    _write_inputs(d, scene, np.concatenate(sets), n, 2, 0, 0, dict(LOOP_RP, heading_mode=mode, seed=seed), inject_p=p)
    r = subprocess.run([facade_exe, "inject", d, str(C_), repr(float(cfg.res))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.split()[0] in ("polar", "cart")]
    assert [(w, int(a)) for w, a in lines] == [("polar", c) for _, c in want] + [("cart", want_cart[0])]
    for i in range(2):
        assert np.fromfile(os.path.join(d, f"out_sensor_polar_{i}.bin"), RR.STATE_DTYPE).tobytes() == want[i][0].tobytes(), i
    assert np.fromfile(os.path.join(d, "out_sensor_cart_0.bin"), RR.STATE_DTYPE).tobytes() == want_cart[1].tobytes()


STEPS = 8


def _sensor_cfg(scene, n, candidates):
    c = _loop_cfg(scene, 1, n)
    c.recovery_candidates = candidates
    return c


def test_cpp_core_python_core_and_handle_loop_agree(K, scene, facade_exe):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd._lib import RecoveryStateC
    from top_down_renderer_amd.particle_filter import FilterParams
    from top_down_renderer_amd.top_down_render_core import TopDownRenderCore
    cfg, n, C_ = scene.cfg, 4096, 8
    st = _spread_states(scene, n, 60, False)
    d = tempfile.mkdtemp(prefix="tdr_sensor_")
    _write_inputs(d, scene, st, n, 1, STEPS, 1, LOOP_RP)
    r = subprocess.run([facade_exe, "loop", d, str(C_)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rec_c, st_c = _read_loop(d, 0, STEPS, n)
    cfgc = _sensor_cfg(scene, n, C_)
    rec_p, st_p = _python_core_trace(K, scene, cfgc, st, STEPS)
    assert rec_c[:, 1].sum() > 0, rec_c                                     # the tracker did ask for injections
    assert np.array_equal(rec_c, rec_p), (rec_c, rec_p)
    assert st_c.tobytes() == st_p.tobytes()
    # the same steps as handle calls; the core's own publishPoseEst steps the range scale over the handle's statistics
    m = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    f = batch.FilterHandle(m, n, FilterParams(fixed_scale=1.0), seed=7)
    f.set_states(st)
    rend = batch.Renderer(scene.lut)
    core = TopDownRenderCore(cfgc)
    state = RecoveryStateC(0.0, 0.0)
    pcl = np.zeros((len(scene.pts), 8), F32)
    pcl[:, :3], pcl[:, 4] = scene.pts[:, :3], scene.pts[:, 3]
    for s in range(STEPS):
        res = float(core.current_range_scale_)
        rend.render_polar(pcl, 8, 4, res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
        f.propagate(*MOTION)
        f.update(rend, res)
        core.filter_ = batch.HandleView(f)
        core.publishPoseEst()
        core.filter_ = None
        got = f.recovery_step_sensor(state, cfgc.recovery, C_, rend, res)
        assert (got[0], float(got[1]), state.w_slow, state.w_fast) == tuple(rec_c[s]), s
        assert f.states().tobytes() == st_c[s].tobytes(), s
    # the uniform injection takes another course from the first injection on
    rec_u, st_u = _python_core_trace(K, scene, _loop_cfg(scene, 1, n), st, STEPS)
    assert st_u.tobytes() != st_p.tobytes()


def test_one_candidate_is_the_loop_without_the_field(K, scene, facade_exe):
    cfg, n = scene.cfg, 2048
    st = _spread_states(scene, n, 61, False)
    rec_a, st_a = _python_core_trace(K, scene, _loop_cfg(scene, 1, n), st, 6)
    rec_b, st_b = _python_core_trace(K, scene, _sensor_cfg(scene, n, 1), st, 6)
    assert rec_a[:, 1].sum() > 0 and np.array_equal(rec_a, rec_b) and st_a.tobytes() == st_b.tobytes()
    out = {}
    for name, exe, extra in (("plain", _build("facade_recovery"), []), ("one", facade_exe, ["1"])):
        d = tempfile.mkdtemp(prefix="tdr_sensor_")
        _write_inputs(d, scene, st, n, 1, 6, 1, LOOP_RP)
        r = subprocess.run([exe, "loop", d] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name] = _read_loop(d, 0, 6, n)
    assert np.array_equal(out["plain"][0], out["one"][0]) and out["plain"][1].tobytes() == out["one"][1].tobytes()
    assert np.array_equal(out["one"][0], rec_a) and out["one"][1].tobytes() == st_a.tobytes()


def test_a_batch_with_more_candidates_is_refused(scene, facade_exe):
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    cfg, n = scene.cfg, 512
    f, r = _handle(scene, "fixed", n, seed=7)
    st = _spread_states(scene, n, 3, False)
    f.set_states(st)
    with pytest.raises(ValueError, match="recovery_candidates"):
        batch.LoopBatch([f], [r], _sensor_cfg(scene, n, 2), float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    batch.LoopBatch([f], [r], _sensor_cfg(scene, n, 1), float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)      # one candidate: built
    c = _sensor_cfg(scene, n, 2)
    c.recovery_every = 0                                           # no recovery step: the field is not read
    batch.LoopBatch([f], [r], c, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    assert f.states().tobytes() == st.tobytes()
    with pytest.raises(ValueError, match="recovery_candidates"):
        pkg.CoreConfig(recovery_every=1, recovery_candidates=5000).check()
    d = tempfile.mkdtemp(prefix="tdr_sensor_")
    _write_inputs(d, scene, st, n, 1, 1, 1, LOOP_RP)
    out = subprocess.run([facade_exe, "batch", d, "2"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("refused:") and "recovery_candidates = 2" in out.stdout, out.stdout + out.stderr
    out = subprocess.run([facade_exe, "batch", d, "1"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["stepped"], out.stdout + out.stderr
