"""GPU: the particle picture (include/tdr.h, "the particle picture"; csrc/tdr_viz.hip) against its NumPy restatement
(tests/viz_ref.py), byte for byte: np.array_equal, no tolerance.  Layer 1 (the three launchers), the C handle
(tdr_filter_set_viz_background / tdr_filter_visualize), the Python filter (setVizBackground / renderViz) and the C++
classes (tests/cpp/facade_viz.cpp)."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import viz_ref as V

from top_down_renderer_amd import STATE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
pytestmark = pytest.mark.gpu
vp = C.c_void_p


def P(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def k():
    from top_down_renderer_amd.kernels import HipKernels
    return HipKernels()


def background(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def states_at(H, pts, thetas=None):
    """Particles whose pt is exactly pts[i] = (px, py) (scale 1, init 0): x = px + 0.5, y = H - py - 0.5."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    st = np.zeros(len(pts), STATE_DTYPE)
    st["dx_m"], st["dy_m"] = pts[:, 0] + 0.5, H - pts[:, 1] - 0.5
    st["theta"] = np.linspace(-3, 3, len(pts)) if thetas is None else thetas
    st["scale"], st["have_init"] = 1.0, 1
    return st


def raw_states(xs, ys, thetas):
    st = np.zeros(len(xs), STATE_DTYPE)
    st["dx_m"], st["dy_m"], st["theta"], st["scale"], st["have_init"] = xs, ys, thetas, 1.0, 1
    return st


def draw(k, st, bg, means=(), covs=(), best=None, arrows=None, pub_scale=1.0):
    """The picture through the layer-1 launchers on torch buffers."""
    import torch
    from top_down_renderer_amd.kernels import viz_overlay_host
    H, W = bg.shape[:2]
    n = len(st)
    dev = k.zeros((7, max(n, 1)))
    if n:
        k.states_to_device(st, dev, n)
    segs = viz_overlay_host(np.asarray(means, F32).reshape(-1, 3), np.asarray(covs, F32).reshape(-1, 3, 3), best, arrows, H)
    oh, ow = V.published_size(H, W, pub_scale)
    out = k.viz_draw(dev, n, k.to_device(bg), k.viz_planes(H, W), segs, oh, ow)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def edge_particles(H, W):
    xs = [0, 31, 32, 33, W - 1, W]
    ys = [0, H - 1, H]
    pts = [(x, y) for x in xs for y in ys] + [(0, 0), (W, 0), (0, H), (W, H), (W - 1, H - 1)]
    pts += [(x, H // 2) for x in range(0, W + 1, 5)] + [(W // 2, y) for y in range(0, H + 1, 5)]   # clipped on every edge
    st = states_at(H, pts)
    # dots from each side, and from coordinates that convert to INT_MIN
    out = raw_states([-3.0, W + 1.5, W / 2, W / 3, -50.0, W + 70.0, np.nan, np.inf, -np.inf, 1e20, 4.0, 7.0],
                     [H / 2, H / 3, -2.0, H + 1.5, -50.0, H + 70.0, 5.0, 5.0, np.nan, -1e20, np.inf, -np.inf],
                     np.linspace(0, 6, 12))
    return np.concatenate([st, out])


MIX_MEANS = np.asarray([[20.5, 18.25, 0.3], [12, 9, 1.0], [25, 22, 2.0]], F32)
MIX_COVS = np.asarray([[[30, 5, 0], [5, 12, 0], [0, 0, 1]],
                       [[10, -3, 0], [-3, 4, 0], [0, 0, 1]],
                       [[9, 0, 0], [0, 9, 0], [0, 0, 1]]], F32)


# ---- word and row boundaries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(37, 29), (64, 33), (257, 131), (40, 48), (21, 64)])   # the last two: the 16-pixel compose
def test_word_and_row_boundaries(k, H, W):
    st, bg = edge_particles(H, W), background(H, W)
    arrows = [[-4, 3, W // 2, H // 2], [W - 3, H - 3, W + 9, H + 2]]
    got = draw(k, st, bg, MIX_MEANS[:1], MIX_COVS[:1], [W / 2, H / 2, 1.0], arrows)
    assert np.array_equal(got, V.render(st, bg, MIX_MEANS[:1], MIX_COVS[:1], [W / 2, H / 2, 1.0], arrows))


# ---- particle counts -----------------------------------------------------------------------------------------------------
def cloud(n, H, W, sigma, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros(n, STATE_DTYPE)
    st["init_x_px"], st["init_y_px"] = W / 2, H / 2
    st["dx_m"], st["dy_m"] = rng.normal(0, sigma, n), rng.normal(0, sigma, n)
    st["theta"] = rng.uniform(-7, 7, n)
    st["scale"] = rng.uniform(0.8, 1.3, n)     # per-particle scales: dx * scale + init rounds twice
    st["have_init"] = 1
    return st


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
def test_particle_counts(k, n):
    H, W = 64, 97
    st, bg = cloud(n, H, W, 30.0, n), background(H, W, 1)     # sigma 30: a good share lands outside, as dots
    assert np.array_equal(draw(k, st, bg), V.render(st, bg))


def test_100003_particles_on_a_1000_x_1000_image(k):
    H = W = 1000
    st = np.concatenate([cloud(90_000, H, W, 3.0, 5), cloud(10_000, H, W, 150.0, 6), edge_particles(H, W)[:3]])
    assert len(st) == 100_003
    bg = background(H, W, 2)
    assert np.array_equal(draw(k, st, bg), V.render(st, bg))


# ---- contention ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every_heading", [True, False])
def test_5000_particles_on_one_pixel(k, every_heading):
    H, W = 37, 67
    th = np.linspace(-math.pi, math.pi, 5000).astype(F32) if every_heading else np.full(5000, 0.7, F32)
    st, bg = states_at(H, [(33, 17)] * 5000, th), background(H, W, 3)
    a, b = draw(k, st, bg), draw(k, st, bg)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(a, V.render(st, bg))


# ---- headings --------------------------------------------------------------------------------------------------------------
def heading_cases():
    th = []
    for kk in range(-5, 6):
        for base in (math.acos(kk / 5), -math.acos(kk / 5), math.asin(kk / 5), math.pi - math.asin(kk / 5)):
            for turn in (-3, -1, 0, 1, 2):
                t = F32(base + 2 * math.pi * turn)
                th += [np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))]
    sweep = np.linspace(-math.pi, math.pi, 97).astype(F32)        # every reachable dir several times
    return np.concatenate([np.asarray(th, F32), sweep, np.asarray([np.nan, np.inf, -np.inf, 1e30, -4e8], F32)])


def test_headings(k):
    th = heading_cases()
    assert len(np.unique(V.dirs(th[np.isfinite(th)]), axis=0)) >= 28
    side = int(math.ceil(math.sqrt(len(th))))
    H = W = 14 * side + 14
    pts = [(14 * (i % side) + 10, 14 * (i // side) + 10) for i in range(len(th))]     # one cell each: nothing hides anything
    st, bg = states_at(H, pts, th), background(H, W, 4)
    assert np.array_equal(draw(k, st, bg), V.render(st, bg))


# ---- overlay -----------------------------------------------------------------------------------------------------------------
NOT_PSD = np.asarray([[1, 5, 0], [5, 1, 0], [0, 0, 1]], F32)
OVERLAYS = {
    "nothing": dict(),
    "one component": dict(means=MIX_MEANS[:1], covs=MIX_COVS[:1]),
    "three components, best, two arrows": dict(means=MIX_MEANS, covs=MIX_COVS, best=[30.5, 12.5, -2.0],
                                               arrows=[[3, 3, 30, 20], [20, 30, 60, 45]]),      # the second partly outside
    "degenerate ellipse": dict(means=MIX_MEANS[:1], covs=np.asarray([[[0.5, 0, 0], [0, 0.3, 0], [0, 0, 1]]], F32)),
    "non-PSD stop": dict(means=MIX_MEANS, covs=np.stack([MIX_COVS[0], NOT_PSD, MIX_COVS[2]]), best=[5, 5, 0.0]),
    "non-finite": dict(means=np.asarray([[np.nan, 5, 1], [9, 9, np.inf]], F32), covs=MIX_COVS[:2], best=[np.inf, 2, 1]),
    "huge": dict(means=MIX_MEANS[:1], covs=np.asarray([[[1e9, 0, 0], [0, 4e3, 0], [0, 0, 1]]], F32),
                 arrows=[[-100000, -50000, 20, 20], [2_000_000, 0, 5, 5]]),
}


@pytest.mark.parametrize("name", sorted(OVERLAYS))
def test_overlay(k, name):
    H, W = 37, 41
    st, bg = cloud(40, H, W, 6.0, 9), background(H, W, 5)
    assert np.array_equal(draw(k, st, bg, **OVERLAYS[name]), V.render(st, bg, **OVERLAYS[name]))


# ---- layer order ---------------------------------------------------------------------------------------------------------------
def test_layer_order_at_one_pixel(k):
    H, W = 30, 34
    bg = background(H, W, 6)
    arrow_particle, dot_particle = states_at(H, [(5, 5)], [0.4]), raw_states([np.nan], [np.nan], [0.0])   # the dot lands on (5, 5)
    best, arrows = [5.5, H - 5.5, 1.0], [[2, 5, 12, 5]]
    layers = [("caller", V.GREEN), ("best", V.BLUE), ("dot", V.GREEN), ("arrow", V.RED), ("background", tuple(bg[5, 5]))]
    present = {"caller", "best", "dot", "arrow"}
    for name, colour in layers:
        st = np.concatenate([arrow_particle[:1 if "arrow" in present else 0], dot_particle[:1 if "dot" in present else 0]])
        kw = dict(best=best if "best" in present else None, arrows=arrows if "caller" in present else None)
        got = draw(k, st, bg, **kw)
        assert tuple(got[5, 5]) == colour, name
        assert np.array_equal(got, V.render(st, bg, **kw)), name
        present.discard(name)


# ---- scales ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(37, 29), (64, 48)])
@pytest.mark.parametrize("s", [1.0, 0.5, 0.2, 0.37, 1.5])
def test_scales(k, H, W, s):
    st, bg = edge_particles(H, W), background(H, W, 7)
    kw = dict(means=MIX_MEANS[:2], covs=MIX_COVS[:2], best=[W / 2, H / 2, 2.0], arrows=[[1, 1, W - 2, H - 2]], pub_scale=s)
    got = draw(k, st, bg, **kw)
    assert got.shape == V.published_size(H, W, s) + (3,)
    assert np.array_equal(got, V.render(st, bg, **kw))


# ---- the C handle, the Python filter ----------------------------------------------------------------------------------------
class Handle:
    """A tdr_map + tdr_filter pair on the scene `sc` through the C ABI."""

    def __init__(self, sc, n, seed=7, comm=None):
        from top_down_renderer_amd import _lib
        from top_down_renderer_amd._lib import check
        import top_down_renderer_amd as pkg
        self.L = L = _lib.load()
        cfg = sc.cfg
        ncls, H, W = sc.class_maps.shape
        self.m, self.f = vp(), vp()
        check(L.tdr_map_create(C.byref(self.m)))
        maps_cm = np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), F32)
        mask_cm = np.ascontiguousarray(sc.class_mask.T, np.uint8)
        check(L.tdr_map_set(self.m, P(maps_cm), P(mask_cm), ncls, H, W, C.c_float(1.0), 0, 0))
        check(L.tdr_map_sample_pts_polar(self.m, cfg.nb, cfg.nr, C.c_float(cfg.ang_res)))
        self.fp = pkg.FilterParams(fixed_scale=1.0).to_c(ncls)
        if comm is None:
            check(L.tdr_filter_create(self.m, n, C.byref(self.fp), seed, C.byref(self.f)))
        else:
            check(L.tdr_filter_create_sharded(self.m, n, C.byref(self.fp), seed, comm, C.byref(self.f)))
        check(L.tdr_filter_configure(self.f, 1, 0))      # the reference-ordered generator, like the Python filter's default
        self.r = vp()
        check(L.tdr_renderer_create(P(np.ascontiguousarray(sc.lut, np.int32)), C.byref(self.r)))
        self.sc = sc

    def step(self):
        """propagate + update on the scene's cloud, the motion step_python makes."""
        from top_down_renderer_amd._lib import check
        sc, cfg, L = self.sc, self.sc.cfg, self.L
        pcl = np.zeros((len(sc.pts), 8), F32)
        pcl[:, :3], pcl[:, 4] = sc.pts[:, :3], sc.pts[:, 3]
        check(L.tdr_filter_propagate(self.f, C.c_float(1.0), C.c_float(0.0), C.c_float(0.01)))
        check(L.tdr_renderer_render(self.r, 1, P(pcl), 8, 4, len(pcl), C.c_float(cfg.res), C.c_float(cfg.ang_res), cfg.ncls,
                                    cfg.nb, cfg.nr, None))
        check(L.tdr_filter_update(self.f, None, self.r, C.c_float(cfg.res), -1))

    def set_states(self, st):
        from top_down_renderer_amd._lib import check
        check(self.L.tdr_filter_set_states(self.f, P(np.ascontiguousarray(st)), len(st)))

    def states(self):
        from top_down_renderer_amd._lib import check
        n = self.L.tdr_filter_num_particles(self.f)
        st = np.zeros(n, STATE_DTYPE)
        check(self.L.tdr_filter_get_states(self.f, P(st), n))
        return st

    def set_background(self, bg):
        return self.L.tdr_filter_set_viz_background(self.f, P(np.ascontiguousarray(bg)), bg.shape[0], bg.shape[1])

    def visualize(self, s, arrows=None, out=None):
        """(rc, image or None): a size query, then the picture into `out` (default: an array of the published size)."""
        arr = None if arrows is None else np.ascontiguousarray(arrows, np.int32)
        m = 0 if arr is None else len(arr)
        oh, ow = C.c_int(-7), C.c_int(-7)
        rc = self.L.tdr_filter_visualize(self.f, C.c_float(s), None if arr is None else P(arr), m, None, 0, C.byref(oh), C.byref(ow))
        if rc != 0:
            assert (oh.value, ow.value) == (-7, -7)
            return rc, None
        if out is None:
            out = np.zeros((oh.value, ow.value, 3), np.uint8)
        rc = self.L.tdr_filter_visualize(self.f, C.c_float(s), None if arr is None else P(arr), m, P(out), out.size, C.byref(oh), C.byref(ow))
        return rc, out

    def close(self):
        self.L.tdr_filter_destroy(self.f)
        self.L.tdr_renderer_destroy(self.r)
        self.L.tdr_map_destroy(self.m)


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene("c1", n_particles=512)


def python_filter(k, sc):
    """The Python filter on the scene's map and particles, with its renderer holding the scene's scan."""
    import top_down_renderer_amd as pkg
    cfg = sc.cfg
    m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
    m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
    r = pkg.ScanRendererPolar(sc.lut, kernels=k)
    r.set_output_shape(cfg.ncls, cfg.nb, cfg.nr)
    r.renderSemanticTopDown(sc.pts, cfg.res, cfg.ang_res)
    f = pkg.ParticleFilter(len(sc.states), m, pkg.FilterParams(fixed_scale=1.0), seed=7, kernels=k, init_particles=False)
    f.set_states(sc.states)
    return f, r, m


def step_python(f, r, sc):
    f.propagate((1.0, 0.0), 0.01)
    f.update(r.last_scan(), None, sc.cfg.res)


def test_handle_python_filter_and_launchers_agree(k, scene):
    from top_down_renderer_amd._lib import check
    sc = scene
    H, W = sc.class_maps.shape[1:]
    bg = background(H, W, 8)
    arrows = [[10, 10, 40, 30], [W - 5, 5, W + 20, 9]]
    f, r, m = python_filter(k, sc)
    h = Handle(sc, len(sc.states))
    try:
        h.set_states(sc.states)
        assert h.set_background(bg) == 0
        f.setVizBackground(bg)
        # before the first update: no best arrow, no mixture
        rc, img = h.visualize(0.5, arrows)
        assert rc == 0 and np.array_equal(img, V.render(sc.states, bg, arrows=arrows, pub_scale=0.5))
        assert np.array_equal(f.renderViz(0.5, arrows), img)
        # one step on both, then the mixture
        h.step()
        step_python(f, r, sc)
        check(h.L.tdr_filter_compute_gmm(h.f))
        f.computeGMM()
        st = h.states()
        assert np.array_equal(st.view(np.uint8), f.get_states().view(np.uint8))
        kk = C.c_int(0)
        means, covs = np.zeros((32, 3), F32), np.zeros((32, 9), F32)
        check(h.L.tdr_filter_get_gmm(h.f, 32, C.byref(kk), P(means), P(covs)))
        means, covs = means[:kk.value], covs[:kk.value].reshape(-1, 3, 3)
        best, cov = np.zeros(4, F32), np.zeros(16, F32)
        check(h.L.tdr_filter_mean_cov(h.f, 1, P(best), P(cov)))
        assert kk.value >= 1
        for s in (1.0, 0.37):
            want = V.render(st, bg, means, covs, best[:3], arrows, s)
            rc, img = h.visualize(s, arrows)
            assert rc == 0 and np.array_equal(img, want)                                    # the C handle
            assert np.array_equal(draw(k, st, bg, means, covs, best[:3], arrows, s), want)  # the layer-1 launchers
            assert np.array_equal(f.renderViz(s, arrows), want)                             # the Python filter
        # a Cartesian filter reads states only: the same picture
        hc = vp()
        check(h.L.tdr_map_set_window(h.m, 8, 8))
        check(h.L.tdr_filter_create_cart(h.m, len(st), C.byref(h.fp), 7, C.byref(hc)))
        check(h.L.tdr_filter_set_states(hc, P(st), len(st)))
        assert h.L.tdr_filter_set_viz_background(hc, P(bg), H, W) == 0
        out, oh, ow = np.zeros((H, W, 3), np.uint8), C.c_int(0), C.c_int(0)
        assert h.L.tdr_filter_visualize(hc, C.c_float(1.0), None, 0, P(out), out.size, C.byref(oh), C.byref(ow)) == 0
        assert np.array_equal(out, V.render(st, bg))
        h.L.tdr_filter_destroy(hc)
    finally:
        h.close()


def test_python_filter_with_a_three_component_mixture(k, scene):
    f, r, m = python_filter(k, scene)
    H, W = scene.class_maps.shape[1:]
    bg = background(H, W, 9)
    f.setVizBackground(bg)
    f.gmm_means_, f.gmm_covs_ = MIX_MEANS.copy(), MIX_COVS.copy()
    assert np.array_equal(f.renderViz(1.0), V.render(scene.states, bg, MIX_MEANS, MIX_COVS))
    for bad in (1e-4, float("nan"), 1e6):
        with pytest.raises(ValueError):
            f.renderViz(bad)


def test_visualize_leaves_the_filter_untouched(k, scene):
    from top_down_renderer_amd._lib import check
    sc = scene
    H, W = sc.class_maps.shape[1:]
    a, b = Handle(sc, len(sc.states)), Handle(sc, len(sc.states))
    try:
        n = len(sc.states)
        for h in (a, b):
            h.set_states(sc.states)
        assert a.set_background(background(H, W, 10)) == 0
        for step in range(4):
            for h in (a, b):
                h.step()
            rc, img = a.visualize(0.5, [[1, 2, 30, 40]])
            assert rc == 0
            check(a.L.tdr_filter_compute_gmm(a.f))
            check(b.L.tdr_filter_compute_gmm(b.f))
            w, idx = np.zeros((2, n), F32), np.zeros((2, n), np.int32)
            for i, h in enumerate((a, b)):
                check(h.L.tdr_filter_get_weights(h.f, P(w[i]), n))
                check(h.L.tdr_filter_get_resample_indices(h.f, P(idx[i]), n))
            assert np.array_equal(w[0].view(np.uint32), w[1].view(np.uint32)) and np.array_equal(idx[0], idx[1])
            assert np.array_equal(a.states().view(np.uint8), b.states().view(np.uint8))
    finally:
        a.close()
        b.close()


def test_refusals_leave_the_output_untouched(k, scene):
    sc = scene
    H, W = sc.class_maps.shape[1:]
    h = Handle(sc, len(sc.states))
    L = h.L
    try:
        h.set_states(sc.states)
        out = np.full((H, W, 3), 0xA5, np.uint8)
        oh, ow = C.c_int(-7), C.c_int(-7)

        def refused(rc, word):
            assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
            assert (out == 0xA5).all()

        L.tdr_set_error(0, b"")
        refused(L.tdr_filter_visualize(h.f, C.c_float(1.0), None, 0, P(out), out.size, C.byref(oh), C.byref(ow)), "background")
        assert (oh.value, ow.value) == (-7, -7)
        small = np.zeros((10, 40, 3), np.uint8)
        refused(L.tdr_filter_set_viz_background(h.f, P(small), 10, 40), "10 x 40")
        refused(L.tdr_filter_set_viz_background(h.f, P(small), 40, 10), "40 x 10")
        refused(L.tdr_filter_visualize(h.f, C.c_float(1.0), None, 0, P(out), out.size, C.byref(oh), C.byref(ow)), "background")
        assert h.set_background(background(H, W, 11)) == 0
        refused(L.tdr_filter_visualize(h.f, C.c_float(1.0), None, 0, P(out), out.size - 1, C.byref(oh), C.byref(ow)), "room")
        assert (oh.value, ow.value) == (H, W)                  # the size is still reported
        refused(L.tdr_filter_visualize(h.f, C.c_float(1e-4), None, 0, P(out), out.size, C.byref(oh), C.byref(ow)), "publishes 0 x 0")
        refused(L.tdr_filter_visualize(h.f, C.c_float(float("nan")), None, 0, P(out), out.size, C.byref(oh), C.byref(ow)), "publishes")
        refused(L.tdr_filter_visualize(h.f, C.c_float(1e4), None, 0, P(out), out.size, C.byref(oh), C.byref(ow)), "publishes")
        assert h.visualize(1.0)[0] == 0                        # and the handle still draws
    finally:
        h.close()
    # a sharded handle (one rank, a caller-supplied transport that is never asked for anything here)
    AG = C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_size_t, vp)
    BC = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, vp)

    class Ops(C.Structure):
        _fields_ = [("ctx", vp), ("all_gather", AG), ("broadcast", BC)]
    ops = Ops(None, AG(lambda *a: 0), BC(lambda *a: 0))
    comm = vp()
    assert L.tdr_comm_create(1, 0, C.byref(ops), C.byref(comm)) == 0
    hs = Handle(sc, len(sc.states), comm=comm)
    try:
        hs.set_states(sc.states)
        assert hs.set_background(background(H, W, 12)) == 0
        rc = L.tdr_filter_visualize(hs.f, C.c_float(1.0), None, 0, P(out), out.size, C.byref(oh), C.byref(ow))
        assert rc == -1 and "sharded" in L.tdr_last_error().decode() and (out == 0xA5).all()
    finally:
        hs.close()
        L.tdr_comm_destroy(comm)


# ---- the C++ classes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade_viz_exe():
    from top_down_renderer_amd import build
    build.build()
    pkg = os.path.join(ROOT, "top_down_renderer_amd")
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_viz")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_viz.cpp"), "-o", exe, "-L", pkg, "-ltdr_hip",
                    f"-Wl,-rpath,{pkg}"], check=True)
    return exe


def test_cpp_classes_draw_the_python_filters_picture(k, scene, facade_viz_exe):
    import top_down_renderer_amd as pkg
    sc = scene
    f, r, m = python_filter(k, sc)
    ncls, rows, cols = sc.class_maps.shape
    H, W, s = 45, 52, 0.5
    st = np.concatenate([cloud(300, H, W, 12.0, 13), edge_particles(H, W)])
    f2 = pkg.ParticleFilter(len(st), m, pkg.FilterParams(fixed_scale=1.0), seed=3, kernels=k, init_particles=False)
    f2.set_states(st)
    bg = background(H, W, 14)
    arrows = np.asarray([[4, 4, 30, 20], [40, 40, 70, 41]], np.int32)
    f2.setVizBackground(bg)
    want, plain = f2.renderViz(s, arrows), f2.renderViz(1.0)
    assert np.array_equal(want, V.render(st, bg, arrows=arrows, pub_scale=s))
    path = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "viz.bin")
    with open(path, "wb") as fh:
        fh.write(np.asarray([ncls, rows, cols, len(st), H, W, len(arrows), want.shape[0], want.shape[1]], np.int32).tobytes())
        fh.write(np.asarray([s], F32).tobytes())
        fh.write(np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), F32).tobytes())
        fh.write(np.ascontiguousarray(sc.class_mask.T, np.uint8).tobytes())
        fh.write(st.tobytes() + bg.tobytes() + arrows.tobytes() + want.tobytes() + plain.tobytes())
    out = subprocess.run([facade_viz_exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", str(want.shape[0]), str(want.shape[1])], out.stdout
