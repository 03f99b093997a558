"""GPU: the pose-grid search (include/tdr.h, "pose-grid search") through the facades: the handle, the Python filter on torch
buffers and the C++ classes (tests/cpp/facade_grid.cpp) give the same planes, peaks and, after injectCells of the peaks'
cells, the same particle sets."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import grid_ref as GR
import recovery_ref as RR
from test_recovery import LOOP_RP, _handle, _spread_states, _write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32
N, P, SEED, R, KP = 2048, 0.25, 900, 2, 8


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


@pytest.fixture(scope="module")
def facade_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_grid")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_grid.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip", f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def _search_and_inject(f, scan, res, spec, mode):
    g = f.grid_search(scan, res, spec, R, KP, vol=True) if hasattr(f, "grid_search") else f.gridSearch(scan, res, spec, R, KP, vol=True)
    inject = f.inject_cells if hasattr(f, "inject_cells") else f.injectCells
    cnt = inject(g.peaks["cell"], P, mode, SEED)
    return g, cnt, (f.states() if hasattr(f, "states") else f.get_states())


def _same(a, b):
    assert (a.listed, a.n_peaks) == (b.listed, b.n_peaks)
    assert a.w.tobytes() == b.w.tobytes() and a.theta.tobytes() == b.theta.tobytes() and a.vol.tobytes() == b.vol.tobytes()
    assert a.peaks.tobytes() == b.peaks.tobytes()


@pytest.mark.parametrize("mode,H", [(0, 1), (1, 5)])
def test_handle_python_filter_and_cpp_classes_agree(K, scene, facade_exe, mode, H):
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib, batch
    cfg = scene.cfg
    sp = GR.Spec(2, 2, 4, 75, 75, road_only=1, heading_mode=mode, n_headings=H, theta0=-1.0, dtheta=0.5, scale=1.0)
    spec = _lib.grid_spec(*sp)
    states = _spread_states(scene, N, 20, False)
    # the handle: a polar filter, and a Cartesian one over the window the C++ program sets
    f, rend = _handle(scene, "fixed", N, seed=7)
    f.set_states(states)
    hg, hcnt, hst = _search_and_inject(f, rend, cfg.res, spec, mode)
    assert hg.listed == len(GR.lattice_list(scene.class_maps, sp)) > 500 and hg.n_peaks >= KP and len(hg.peaks) == KP
    assert N * P / 2 < hcnt < 2 * N * P
    mc = batch.MapHandle(scene.class_maps, scene.class_mask, cfg.map_resolution)
    mc.set_window(cfg.nb, cfg.nr)
    rc = batch.Renderer(scene.lut)
    rc.render_cart(scene.pts, 4, 3, cfg.res, cfg.ncls, cfg.nb, cfg.nr)
    fc = batch.FilterHandle(mc, N, pkg.FilterParams(fixed_scale=1.0), seed=7, cart=True)
    fc.set_states(states)
    cg, ccnt, cst = _search_and_inject(fc, rc, cfg.res, spec, mode)
    # the Python filter on torch buffers
    m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    rp = pkg.ScanRendererPolar(scene.lut, kernels=K)
    rp.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    rp.renderSemanticTopDown(scene.pts, cfg.res, cfg.ang_res)
    pf = pkg.ParticleFilter(N, m, pkg.FilterParams(fixed_scale=1.0), seed=1, kernels=K, init_particles=False)
    pf.set_states(states)
    pg, pcnt, pst = _search_and_inject(pf, rp.last_scan(), cfg.res, spec, mode)
    _same(pg, hg)
    assert pcnt == hcnt and pst.tobytes() == hst.tobytes() and pf._maybe_uninit == (mode == 0)
    for bad in (dict(res=0.0), dict(res=float("nan"))):
        with pytest.raises(ValueError):
            pf.gridSearch(rp.last_scan(), bad["res"], spec)
    for cells, p in (([], 0.5), ([cfg.map_size ** 2], 0.5), ([5], 1.5)):
        with pytest.raises(ValueError):
            pf.injectCells(np.array(cells, np.uint32), p)
    assert pf.get_states().tobytes() == hst.tobytes()
    # ParticleFilter::gridSearch / injectCells, ParticleFilterCartesian::gridSearch / injectCells
    d = tempfile.mkdtemp(prefix="tdr_grid_")
    _write_inputs(d, scene, states, N, 1, 0, 0, dict(LOOP_RP, heading_mode=mode, seed=SEED), inject_p=P)
    args = [repr(float(cfg.res))] + [repr(float(v)) if isinstance(v, float) else str(v) for v in sp] + [str(R), str(KP)]
    r = subprocess.run([facade_exe, d] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.split()[0] in ("polar", "cart", "refused")}
    assert lines == {"polar": [hg.listed, hg.n_peaks, hcnt], "cart": [cg.listed, cg.n_peaks, ccnt], "refused": [3]}
    for who, g, st in (("polar", hg, hst), ("cart", cg, cst)):
        rd = lambda name, dt: np.fromfile(os.path.join(d, f"out_grid_{who}_{name}.bin"), dt)
        assert rd("w", F32).tobytes() == g.w.tobytes() and rd("theta", F32).tobytes() == g.theta.tobytes(), who
        assert rd("vol", F32).tobytes() == g.vol.tobytes() and rd("peaks", _lib.GRID_PEAK_DTYPE).tobytes() == g.peaks.tobytes(), who
        assert rd("states", RR.STATE_DTYPE).tobytes() == st.tobytes(), who


@pytest.mark.parametrize("mode,H", [(0, 1), (1, 5)])
@pytest.mark.parametrize("kind", ["cart", "polar"])
def test_python_filter_equals_the_handle_on_cartesian_and_free_scale_filters(K, scene, kind, mode, H):
    """The Python filter's Cartesian launches (the heading search, the order by pose, the scoring) and its free-scale polar
    case (no uniform scale goes to the launch) against the handle: the same planes, peaks and injected sets."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib
    cfg = scene.cfg
    spec = _lib.grid_spec(2, 2, 4, 75, 75, 1, mode, H, -1.0, 0.5, 1.25 if kind == "polar" else 1.0)
    states = _spread_states(scene, N, 21, True)                              # every particle its own scale
    f, rend = _handle(scene, kind, N, seed=7)                                # fixed_scale = -1; cart: a 24 x 20 window
    f.set_states(states)
    if kind == "cart":
        img = rend.get_render()[0]                                           # (ncls, 24, 20): both sides pack these images
        hscan, pscan = img, np.ascontiguousarray(img.transpose(0, 2, 1).reshape(cfg.ncls, -1))
        m = pkg.TopDownMap(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
        m.setWindow(24, 20)
    else:
        m = pkg.TopDownMapPolar(pkg.Params(resolution=cfg.map_resolution), scene.class_maps, scene.class_mask, kernels=K)
        m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
        rp = pkg.ScanRendererPolar(scene.lut, kernels=K)
        rp.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
        rp.renderSemanticTopDown(scene.pts, cfg.res, cfg.ang_res)
        hscan, pscan = rend, rp.last_scan()
    hg, hcnt, hst = _search_and_inject(f, hscan, cfg.res, spec, mode)
    assert hg.listed > 500 and hg.n_peaks >= 1 and np.isfinite(hg.w).any()
    pf = pkg.ParticleFilter(N, m, pkg.FilterParams(fixed_scale=-1.0), seed=1, kernels=K, init_particles=False)
    pf.set_states(states)
    pg, pcnt, pst = _search_and_inject(pf, pscan, cfg.res, spec, mode)
    _same(pg, hg)
    assert pcnt == hcnt and pst.tobytes() == hst.tobytes(), (kind, mode)
    # a spec outside its ranges raises before the scan is packed
    for bad in (dict(step=0), dict(nx=0), dict(n_headings=0), dict(scale=0.0)):
        sp = _lib.grid_spec(2, 2, 4, 75, 75, 1, mode, H, -1.0, 0.5, 1.0)
        for name, v in bad.items():
            setattr(sp, name, v)
        with pytest.raises(ValueError):
            pf.gridSearch(object(), cfg.res, sp)
    for kw in (dict(nms_radius=17), dict(max_peaks=4097)):
        with pytest.raises(ValueError):
            pf.gridSearch(object(), cfg.res, spec, **kw)
    assert pf.get_states().tobytes() == hst.tobytes()
