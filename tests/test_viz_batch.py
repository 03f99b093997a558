"""GPU: the batched pictures.  tdr_batch_visualize against per-filter tdr_filter_visualize and tdr_batch_scan_pictures
against per-renderer tdr_renderer_visualize, byte for byte — the project's test of every batched call — with the
refusals, batch.LoopBatch's pictures against robots stepped alone, and the C++ classes (tests/cpp/facade_pictures.cpp)."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import scan_viz_ref as S

from top_down_renderer_amd import STATE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
F32 = np.float32
pytestmark = pytest.mark.gpu
vp = C.c_void_p
MOTION = (1.0, 0.0, 0.01)
UNFLATTEN = [3, 200, 17, 255, 0, 9, 31, 32, 33, 64, 65, 127, 128, 129, 254]
LUT = np.random.default_rng(98).integers(0, 256, (256, 3), dtype=np.uint8)


def P(a):
    return a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def L():
    from top_down_renderer_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene("c1", n_particles=512)


def background(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def spread(n, H, W, seed):
    """n particles spread over and beyond an H x W picture (arrows, clipped arrows and border dots)."""
    rng = np.random.default_rng(seed)
    st = np.zeros(n, STATE_DTYPE)
    st["init_x_px"], st["init_y_px"] = W / 2, H / 2
    st["dx_m"], st["dy_m"] = rng.normal(0, 0.4 * W, n), rng.normal(0, 0.4 * H, n)
    st["theta"], st["scale"], st["have_init"] = rng.uniform(-7, 7, n), rng.uniform(0.8, 1.3, n), 1
    return st


def one_pixel(n, x, y, seed):
    st = np.zeros(n, STATE_DTYPE)
    st["dx_m"], st["dy_m"], st["scale"], st["have_init"] = x + 0.5, y + 0.5, 1.0, 1
    st["theta"] = np.random.default_rng(seed).uniform(-math.pi, math.pi, n)
    return st


def three_clumps(n, H, W, seed):
    rng = np.random.default_rng(seed)
    c = np.asarray([[0.25 * W, 0.3 * H], [0.7 * W, 0.35 * H], [0.5 * W, 0.75 * H]])[rng.integers(0, 3, n)]
    st = np.zeros(n, STATE_DTYPE)
    st["dx_m"], st["dy_m"] = c[:, 0] + rng.normal(0, 2.0, n), c[:, 1] + rng.normal(0, 2.0, n)
    st["theta"], st["scale"], st["have_init"] = rng.normal(0.5, 0.1, n), 1.0, 1
    return st


def pcl(p):
    out = np.zeros((len(p), 8), F32)
    out[:, :3], out[:, 4] = p[:, :3], p[:, 3]
    return out


class Fleet:
    """Five filters on one map, and a twin of the first that no batched picture ever touches:
         0  stepped once (a max-likelihood state), then 1024 particles in three clumps and their mixture; background = the map's size
         1  0 particles, 11 x 11
         2  5000 particles on one pixel, 300 x 257
         3  a Cartesian filter, 63 particles spread, 64 x 48
         4  1 particle, 11 x 11 (another image than filter 1's)"""

    def __init__(self, sc):
        import top_down_renderer_amd as pkg
        from top_down_renderer_amd import batch
        cfg = sc.cfg
        ncls, H, W = sc.class_maps.shape
        self.m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
        self.m.sample_pts_polar(cfg.nb, cfg.nr, cfg.ang_res)
        self.m.set_window(8, 8)
        params = pkg.FilterParams(fixed_scale=1.0)
        self.r = batch.Renderer(sc.lut)
        self.r.render_polar(pcl(sc.pts), 8, 4, cfg.res, cfg.ang_res, cfg.ncls, cfg.nb, cfg.nr)

        def mixture_filter():
            f = batch.FilterHandle(self.m, 1024, params, seed=7)
            f.configure(1)
            f.set_states(sc.states)
            f.propagate(*MOTION)
            f.update(self.r, cfg.res)
            f.set_states(three_clumps(1024, H, W, 3))
            f.set_num_gaussians(2)                              # the fit tries 2 and 3 components and keeps 3
            f.compute_gmm()
            f.set_viz_background(background(H, W, 20))
            return f

        self.f = [mixture_filter()]
        self.twin = mixture_filter()
        self.f.append(batch.FilterHandle(self.m, 64, params, seed=8))
        self.f[1].set_viz_background(background(11, 11, 21))
        self.f.append(batch.FilterHandle(self.m, 5000, params, seed=9))
        self.f[2].set_states(one_pixel(5000, 150, 100, 4))
        self.f[2].set_viz_background(background(300, 257, 22))
        self.f.append(batch.FilterHandle(self.m, 63, params, seed=10, cart=True))
        self.f[3].set_states(spread(63, 64, 48, 5))
        self.f[3].set_viz_background(background(64, 48, 23))
        self.f.append(batch.FilterHandle(self.m, 1, params, seed=11))
        self.f[4].set_states(spread(1, 6, 6, 6))
        self.f[4].set_viz_background(background(11, 11, 24))
        self.arrows = [[[10, 10, 40, 30], [W - 5, 5, W + 20, 9]], None, [[3, 3, 250, 200]],
                       [[1, 1, 30, 30], [40, 5, 5, 40], [-9, 20, 70, 21]], []]


@pytest.fixture(scope="module")
def fleet(scene):
    return Fleet(scene)


def test_the_fleet_is_what_the_tests_need(fleet):
    assert [f.num_particles() for f in fleet.f] == [1024, 0, 5000, 63, 1]
    means, covs = fleet.f[0].get_gmm()
    assert len(means) == 3                                     # a three-component mixture
    fleet.f[0].mean_cov(about_max=True)                        # and a max-likelihood state (raises without one)


def snapshot(f):
    n = f.num_particles()
    return n, (f.states().tobytes() if n else b"")


@pytest.mark.parametrize("s", [1.0, 0.5, 0.37])
@pytest.mark.parametrize("K", [1, 2, 5])
def test_batch_visualize_equals_filter_visualize(fleet, K, s):
    from top_down_renderer_amd import batch
    fs, arrows = fleet.f[:K], fleet.arrows[:K]
    before = [snapshot(f) for f in fs]
    want = [f.visualize(s, a) for f, a in zip(fs, arrows)]
    got = batch.visualize_batch(fs, s, arrows)
    again = batch.visualize_batch(fs, s, arrows)
    for i in range(K):
        assert got[i].shape == want[i].shape, i                # out_h, out_w
        assert np.array_equal(got[i], want[i]), i
        assert got[i].tobytes() == again[i].tobytes(), i
    assert [snapshot(f) for f in fs] == before
    if K == 5:      # the pictures are of different things
        assert not np.array_equal(got[1], got[4]) and len({g.shape for g in got}) >= 3


def test_batch_visualize_in_another_order_and_on_a_stream(fleet):
    import torch
    from top_down_renderer_amd import batch
    order = [4, 2, 0, 3, 1]
    fs, arrows = [fleet.f[i] for i in order], [fleet.arrows[i] for i in order]
    want = [f.visualize(0.5, a) for f, a in zip(fs, arrows)]
    stream = torch.cuda.Stream()
    got = batch.visualize_batch(fs, 0.5, arrows, stream=stream.cuda_stream)
    for i in range(5):
        assert np.array_equal(got[i], want[i]), i
    # one request only asks for its size
    arr = (vp * 2)(fs[0].h, fs[1].h)
    from top_down_renderer_amd._lib import VizRequestC, check
    req = (VizRequestC * 2)()
    out = np.zeros_like(want[1])
    req[1].out_bgr_host, req[1].capacity = out.ctypes.data, out.size
    check(fleet.f[0].L.tdr_batch_visualize(arr, 2, C.c_float(0.5), req, None))
    assert (req[0].out_h, req[0].out_w) == want[0].shape[:2] and np.array_equal(out, fs[1].visualize(0.5))   # (no arrows)


def test_batch_visualize_leaves_the_filters_untouched(fleet, scene):
    """States, weights and the generator's position: after batched pictures the filter steps exactly like its twin."""
    from top_down_renderer_amd import batch
    f, t = fleet.f[0], fleet.twin
    batch.visualize_batch(fleet.f, 0.5, fleet.arrows)
    batch.visualize_batch([f], 1.0, [None])
    assert f.states().tobytes() == t.states().tobytes()
    for g in (f, t):
        g.propagate(*MOTION)
        g.update(fleet.r, scene.cfg.res)
    assert f.states().tobytes() == t.states().tobytes() and f.weights().tobytes() == t.weights().tobytes()
    assert f.resample_indices().tobytes() == t.resample_indices().tobytes()
    assert np.array_equal(f.visualize(0.5), t.visualize(0.5))


def test_best_arrow_on_the_device_equals_the_hosts(L):
    """The max-likelihood arrow is computed in the segments launch as the tabulated Arrow(-dir, dir) moved to pt; the host
    (tdr_viz_overlay_host) computes Arrow(pt - dir, pt + dir).  The same segments, wherever pt lies."""
    H = 4000
    rng = np.random.default_rng(1)
    for theta in np.linspace(-math.pi, math.pi, 181).astype(F32):
        dx, dy = int(F32(math.cos(theta)) * F32(5)), int(-F32(math.sin(theta)) * F32(5))
        tab = np.zeros(12, np.int32)
        assert L.tdr_viz_arrow_host(dx, dy, P(tab)) == 0
        for x, y in [(0.0, float(H)), (3999.5, 0.5), (float(rng.integers(0, 1 << 20)), float(-rng.integers(0, 1 << 19)))]:
            best = np.asarray([x, y, theta], F32)
            segs, n = np.zeros((6, 5), np.int32), C.c_int(0)
            assert L.tdr_viz_overlay_host(None, None, 0, P(best), None, 0, H, P(segs), 6, C.byref(n)) == 0
            if n.value == 0:
                continue
            cx, cy = int(best[0]), int(F32(H) - best[1])
            if (segs[0, 2] - segs[0, 0], segs[0, 3] - segs[0, 1]) != (2 * dx, 2 * dy):
                continue                                       # (the library's cosf rounded the other way at a boundary)
            moved = tab.reshape(3, 4) + np.asarray([cx, cy, cx, cy], np.int32)
            assert n.value == 3 and np.array_equal(segs[:3, :4], moved), (theta, x, y)


def test_batch_visualize_refusals_leave_every_output_untouched(fleet, scene, L):
    import test_viz as TV
    from top_down_renderer_amd._lib import VizRequestC
    fs = fleet.f
    shapes = [f.visualize(0.5).shape for f in fs]
    outs = [np.full(sh, 0xA5, np.uint8) for sh in shapes]

    def requests(k=5):
        req = (VizRequestC * k)()
        for i in range(k):
            req[i].out_bgr_host, req[i].capacity, req[i].out_h, req[i].out_w = outs[i].ctypes.data, outs[i].size, -7, -7
        return req

    def refused(rc, word, req):
        assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
        assert all((o == 0xA5).all() for o in outs)
        assert all((q.out_h, q.out_w) == (-7, -7) for q in req)

    arr = (vp * 5)(*[f.h for f in fs])
    s = C.c_float(0.5)
    req = requests()
    refused(L.tdr_batch_visualize(arr, 0, s, req, None), "k = 0", req)
    refused(L.tdr_batch_visualize(None, 5, s, req, None), "null filter array", req)
    refused(L.tdr_batch_visualize(arr, 5, s, None, None), "null request array", req)
    refused(L.tdr_batch_visualize((vp * 5)(fs[0].h, fs[1].h, None, fs[3].h, fs[4].h), 5, s, req, None), "filter 2 is null", req)
    refused(L.tdr_batch_visualize((vp * 5)(fs[0].h, fs[1].h, fs[2].h, fs[0].h, fs[4].h), 5, s, req, None), "twice", req)
    for bad, word in ((1e-4, "publishes 0 x 0"), (math.nan, "publishes"), (1e4, "publishes")):
        refused(L.tdr_batch_visualize(arr, 5, C.c_float(bad), req, None), word, req)
    req[3].capacity -= 1                                       # too little room in one request: nothing is drawn for any
    refused(L.tdr_batch_visualize(arr, 5, s, req, None), "request 3: the image needs", req)
    req = requests()
    req[2].m = 1                                               # arrows announced, none given
    refused(L.tdr_batch_visualize(arr, 5, s, req, None), "request 2: bad arrows", req)
    req = requests()
    # a filter without a background
    from top_down_renderer_amd import batch
    import top_down_renderer_amd as pkg
    bare = batch.FilterHandle(fleet.m, 16, pkg.FilterParams(fixed_scale=1.0), seed=3)
    refused(L.tdr_batch_visualize((vp * 5)(fs[0].h, fs[1].h, fs[2].h, fs[3].h, bare.h), 5, s, req, None), "filter 4 has no background", req)
    # a sharded filter (one rank, a caller-supplied transport that is never asked for anything here)
    AG = C.CFUNCTYPE(C.c_int, vp, vp, vp, C.c_size_t, vp)
    BC = C.CFUNCTYPE(C.c_int, vp, vp, C.c_size_t, C.c_int, vp)

    class Ops(C.Structure):
        _fields_ = [("ctx", vp), ("all_gather", AG), ("broadcast", BC)]
    ops = Ops(None, AG(lambda *a: 0), BC(lambda *a: 0))
    comm = vp()
    assert L.tdr_comm_create(1, 0, C.byref(ops), C.byref(comm)) == 0
    hs = TV.Handle(scene, len(scene.states), comm=comm)
    try:
        hs.set_states(scene.states)
        assert hs.set_background(background(40, 40, 1)) == 0
        refused(L.tdr_batch_visualize((vp * 5)(fs[0].h, hs.f, fs[2].h, fs[3].h, fs[4].h), 5, s, req, None), "filter 1 is sharded", req)
    finally:
        hs.close()
        L.tdr_comm_destroy(comm)
    # and the batch still draws
    assert L.tdr_batch_visualize(arr, 5, s, req, None) == 0
    assert [(q.out_h, q.out_w) for q in req] == [sh[:2] for sh in shapes]
    assert all(np.array_equal(o, f.visualize(0.5)) for o, f in zip(outs, fs))


# ---- the scan pictures ---------------------------------------------------------------------------------------------------------
def scan_cloud(n, reach, nlabels, seed):
    rng = np.random.default_rng(seed)
    pts = np.zeros((n, 8), F32)
    pts[:, :2] = rng.uniform(-reach, reach, (n, 2))
    pts[:, 4] = rng.integers(0, nlabels, n)
    return pts


@pytest.mark.parametrize("nb,nr,ncls", [(100, 25, 6), (33, 65, 2)])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_batch_scan_pictures_equal_renderer_visualize(K, nb, nr, ncls):
    from top_down_renderer_amd import batch
    lut = (np.arange(256) % ncls).astype(np.int32)
    rs = [batch.Renderer(lut) for _ in range(K)]
    clouds = [(scan_cloud(300 * (i + 1), 0.4 * nr, 2 * ncls, i), 8, 4) for i in range(K)]
    half = K // 2                                              # some rendered in a batch, the others alone
    if half:
        batch.render_batch(rs[:half], clouds[:half], 1.0, 2 * math.pi / nb, ncls, nb, nr)
    for r, (pts, stride, ioff) in zip(rs[half:], clouds[half:]):
        r.render_polar(pts, stride, ioff, 1.0, 2 * math.pi / nb, ncls, nb, nr)
    got = batch.scan_pictures_batch(rs, UNFLATTEN[:ncls], LUT)
    assert got.shape == (K, nr, nb, 3)
    for i, r in enumerate(rs):
        want = r.picture(UNFLATTEN[:ncls], LUT)
        assert np.array_equal(got[i], want), i
        imgs = np.ascontiguousarray(np.transpose(r.get_render()[0], (0, 2, 1))).reshape(ncls, -1)
        assert imgs.max() > 0 and np.array_equal(want, S.scan_picture(imgs, nb, nr, UNFLATTEN[:ncls], LUT)), i
    assert np.array_equal(batch.scan_pictures_batch(rs, UNFLATTEN[:ncls], LUT), got)


def test_batch_scan_pictures_refusals(L):
    from top_down_renderer_amd import batch
    ncls, nb, nr = 6, 100, 25
    lut = (np.arange(256) % ncls).astype(np.int32)
    rs = [batch.Renderer(lut) for _ in range(3)]
    for i, r in enumerate(rs[:2]):
        r.render_polar(scan_cloud(500, 10.0, 12, i), 8, 4, 1.0, 2 * math.pi / nb, ncls, nb, nr)
    unf = np.asarray(UNFLATTEN[:ncls], np.int32)
    out = np.full((3, nr, nb, 3), 0xA5, np.uint8)

    def refused(rc, word):
        assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
        assert (out == 0xA5).all()

    arr = (vp * 3)(*[r.h for r in rs])
    refused(L.tdr_batch_scan_pictures(arr, 0, P(unf), P(LUT), P(out), None), "k = 0")
    refused(L.tdr_batch_scan_pictures(None, 2, P(unf), P(LUT), P(out), None), "null")
    refused(L.tdr_batch_scan_pictures(arr, 2, None, P(LUT), P(out), None), "null")
    refused(L.tdr_batch_scan_pictures(arr, 2, P(unf), P(LUT), None, None), "null")
    refused(L.tdr_batch_scan_pictures((vp * 2)(rs[0].h, None), 2, P(unf), P(LUT), P(out), None), "renderer 1 is null")
    refused(L.tdr_batch_scan_pictures((vp * 2)(rs[0].h, rs[0].h), 2, P(unf), P(LUT), P(out), None), "twice")
    refused(L.tdr_batch_scan_pictures(arr, 3, P(unf), P(LUT), P(out), None), "renderer 2 has no render")
    rs[2].render_polar(scan_cloud(500, 10.0, 12, 5), 8, 4, 1.0, 2 * math.pi / 33, ncls, 33, 65)
    refused(L.tdr_batch_scan_pictures(arr, 3, P(unf), P(LUT), P(out), None), "renderer 2 holds a 6x33x65 render")
    assert L.tdr_batch_scan_pictures(arr, 2, P(unf), P(LUT), P(out), None) == 0
    assert np.array_equal(out[0], rs[0].picture(unf, LUT)) and np.array_equal(out[1], rs[1].picture(unf, LUT))
    assert (out[2] == 0xA5).all()


# ---- the batched node loop ----------------------------------------------------------------------------------------------------
def test_loop_batch_pictures_equal_robots_stepped_alone(scene):
    """Three robots, two steps: after each, LoopBatch's scan pictures and particle pictures equal those of three robots
    stepped alone on their own handles (render, propagate, update, mixture; tdr_renderer_visualize, tdr_filter_visualize)."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.top_down_render_core import CoreConfig, TopDownRenderCore
    sc, cfg = scene, scene.cfg
    ncls, nb, nr = cfg.ncls, cfg.nb, cfg.nr
    H, W = sc.class_maps.shape[1:]
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(nb, nr, cfg.ang_res)
    params = pkg.FilterParams(fixed_scale=1.0)
    lab = np.random.default_rng(7).integers(0, 256, (37, 53), dtype=np.uint8)
    rng = np.random.default_rng(11)
    fb, ft, rb, rt, clouds = [], [], [], [], []
    for i in range(3):
        st = sc.states.copy()
        st["dx_m"] += rng.normal(0, 0.5, len(st)).astype(F32)
        for fl in (fb, ft):
            f = batch.FilterHandle(m, len(st), params, seed=31 + i)
            f.configure(1)
            f.set_states(st)
            if i == 2:
                f.set_viz_background(labels=lab, lut=LUT)      # one robot draws on a label background
            else:
                f.set_viz_background(background(H if i == 0 else 64, W if i == 0 else 48, 50 + i))
            fl.append(f)
        rb.append(batch.Renderer(sc.lut))
        rt.append(batch.Renderer(sc.lut))
        keep = rng.random(len(sc.pts)) < 0.9
        clouds.append((pcl(sc.pts[keep]), 8, 4))
    ccfg = CoreConfig(theta_bins=nb, range_bins=nr)
    loop = batch.LoopBatch(fb, rb, ccfg, cfg.ang_res, ncls, nb, nr)
    cores = [TopDownRenderCore(ccfg) for _ in range(3)]
    arrows = [[[5, 5, 40, 20]], None, [[1, 2, 30, 30], [20, 3, 3, 20]]]
    unf = UNFLATTEN[:ncls]
    for step in range(2):
        loop.take_step(clouds, [MOTION] * 3)
        batch.compute_gmm_batch(fb)
        scans, parts = loop.scan_pictures(unf, LUT), loop.particle_pictures(0.5, arrows)
        for i in range(3):
            c = cores[i]                                        # one robot's loop, as tests/test_batch_loop.py steps its twins
            c.last_res_ = c.current_range_scale_
            res = float(c.current_range_scale_)
            pts, stride, ioff = clouds[i]
            rt[i].render_polar(pts, stride, ioff, res, cfg.ang_res, ncls, nb, nr)
            ft[i].propagate(*MOTION)
            ft[i].update(rt[i], res)
            c.filter_ = batch.HandleView(ft[i])
            c.publishPoseEst()
            c.filter_ = None
            ft[i].compute_gmm()
            assert ft[i].states().tobytes() == fb[i].states().tobytes(), (step, i)
            assert np.array_equal(scans[i], rt[i].picture(unf, LUT)), (step, i)
            assert np.array_equal(parts[i], ft[i].visualize(0.5, arrows[i])), (step, i)
        assert scans.shape == (3, nr, nb, 3) and scans.max() > 0


# ---- the C++ classes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade_pictures_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_pictures")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_pictures.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip",
                    f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def test_cpp_classes_draw_the_pictures(scene, facade_pictures_exe):
    """ScanRendererPolar::renderViz / renderVizAnalog, tdr_viz::scanPicture at the node's two call sites, the label
    background, ParticleFilterBatch::renderViz and TopDownRenderCoreBatch::renderPictures after one batched step of two
    robots: the images the program writes back equal the NumPy restatements of what it says they are pictures of."""
    import viz_ref as V
    sc, cfg = scene, scene.cfg
    ncls, rows, cols = sc.class_maps.shape
    nb, nr = cfg.nb, cfg.nr
    pub_scale, analog_scale = 0.5, 0.37
    d = tempfile.mkdtemp(prefix="tdr_pictures_")
    rng = np.random.default_rng(17)
    bg0 = background(rows, cols, 60)
    lab1 = rng.integers(0, 256, (64, 48), dtype=np.uint8)
    packed = rng.integers(0, 1 << 24, 256).astype(np.uint32)
    lut = np.stack([(packed >> 16) & 255, (packed >> 8) & 255, packed & 255], axis=1).astype(np.uint8)   # unpackColor as {B, G, R}
    unf = np.asarray(UNFLATTEN[:ncls], np.int32)
    arrows = [np.asarray([[5, 5, 40, 20], [cols - 4, 3, cols + 9, 8]], np.int32), np.zeros((0, 4), np.int32)]
    open(os.path.join(d, "meta.txt"), "w").write(
        f"{ncls} {rows} {cols} {nb} {nr} {pub_scale} {analog_scale} {rows} {cols} 64 48\n")
    np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), F32).tofile(os.path.join(d, "maps.bin"))
    np.ascontiguousarray(sc.class_mask.T, np.uint8).tofile(os.path.join(d, "mask.bin"))
    packed.tofile(os.path.join(d, "lut.bin"))
    unf.tofile(os.path.join(d, "unflatten.bin"))
    bg0.tofile(os.path.join(d, "bg_0.bin"))
    lab1.tofile(os.path.join(d, "labels_1.bin"))
    for r in range(2):
        st = sc.states.copy()
        st["dx_m"] += rng.normal(0, 0.5, len(st)).astype(F32)
        st.tofile(os.path.join(d, f"states_{r}.bin"))
        pcl(sc.pts[rng.random(len(sc.pts)) < 0.9]).tofile(os.path.join(d, f"pts_{r}.bin"))
        arrows[r].tofile(os.path.join(d, f"arrows_{r}.bin"))
    out = subprocess.run([facade_pictures_exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", str(nr), str(nb)], out.stdout

    def rd(name, dtype):
        return np.fromfile(os.path.join(d, name), dtype)

    bgs = [bg0, S.label_picture(lab1, lut)]
    for r in range(2):
        imgs = rd(f"out_imgs_{r}.bin", F32).reshape(ncls, nb * nr)
        assert imgs.max() > 0
        assert np.array_equal(rd(f"out_scan_{r}.bin", np.uint8).reshape(nr, nb, 3), S.scan_picture(imgs, nb, nr, unf, lut)), r
        assert np.array_equal(rd(f"out_analog_{r}.bin", np.uint8).reshape(nr, nb, 3), S.analog_picture(imgs[r], nb, nr, analog_scale)), r
        assert np.array_equal(rd(f"out_geo_{r}.bin", np.uint8).reshape(nr, nb, 3), S.scan_picture(imgs[:2], nb, nr, unf, lut)), r
        st, best = rd(f"out_states_{r}.bin", STATE_DTYPE), rd(f"out_best_{r}.bin", F32)
        want = V.render(st, bgs[r], best=best[:3], arrows=arrows[r] if len(arrows[r]) else None, pub_scale=pub_scale)
        h, w = rd(f"out_part_size_{r}.bin", np.int32)
        assert (h, w) == want.shape[:2]
        assert np.array_equal(rd(f"out_part_{r}.bin", np.uint8).reshape(h, w, 3), want), r
