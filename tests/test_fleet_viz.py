"""GPU: the fleet picture (include/tdr.h, "the fleet picture"; tdr_k_viz_compose_fleet in csrc/tdr_viz.hip,
tdr_map_set_viz_background*, tdr_batch_visualize_fleet) against its NumPy restatement (tests/fleet_viz_ref.py), byte for
byte: np.array_equal, no tolerance.  The backgrounds are the smallest that reach each form of the compose launch: 11 x 11
(the minimum), 37 x 45 (per-pixel copy), 48 x 64 (16 pixels a thread), 40 x 144 (a plane row of two 16-byte groups,
16 pixels a thread), 33 x 130 (two groups, per-pixel copy); every other published size takes the resample."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import fleet_viz_ref as FV
import numpy as np
import pytest
import scan_viz_ref as S
import viz_ref as V

from top_down_renderer_amd import STATE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
F32 = np.float32
pytestmark = pytest.mark.gpu
vp = C.c_void_p
MOTION = (1.0, 0.0, 0.01)
BACKGROUNDS = [(11, 11), (37, 45), (48, 64), (40, 144), (33, 130)]
SCALES = [1.0, 0.5, 0.37, 1.7]


def P(a):
    return a.ctypes.data_as(vp)


def palette(k, seed=1):
    """k x 3 distinct colours, none of them the caller's green."""
    pal = np.random.default_rng(seed).integers(0, 256, (k, 3, 3), dtype=np.uint8)
    pal[:, :, 2] |= 1                                        # (green has red = 0)
    return pal


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


def states_at(H, pts, thetas):
    """Particles whose pt is exactly pts[i] = (px, py) (scale 1, init 0)."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    st = np.zeros(len(pts), STATE_DTYPE)
    st["dx_m"], st["dy_m"], st["theta"] = pts[:, 0] + 0.5, H - pts[:, 1] - 0.5, thetas
    st["scale"], st["have_init"] = 1.0, 1
    return st


def three_clumps(n, seed):
    """Three clumps of standard deviation 3, the first around (9, 18): its ellipse crosses the column of the left dots."""
    rng = np.random.default_rng(seed)
    c = np.asarray([[9.0, 18.0], [31.0, 12.0], [22.0, 28.0]])[rng.integers(0, 3, n)]
    st = np.zeros(n, STATE_DTYPE)
    st["dx_m"], st["dy_m"] = c[:, 0] + rng.normal(0, 3.0, n), c[:, 1] + rng.normal(0, 3.0, n)
    st["theta"], st["scale"], st["have_init"] = rng.normal(0.5, 0.1, n), 1.0, 1
    return st


def pcl(p):
    out = np.zeros((len(p), 8), F32)
    out[:, :3], out[:, 4] = p[:, :3], p[:, 3]
    return out


def robot(f):
    """What the restatement needs of a filter, read back: states, the mixture, the max-likelihood state if there is one."""
    from top_down_renderer_amd._lib import TdrError
    means, covs = f.get_gmm()
    n = f.num_particles()
    try:
        best = f.mean_cov(about_max=True)[0][:3] if n else None        # (without particles the call answers zeros)
    except TdrError:
        best = None                                                    # before the first update
    return {"st": f.states() if n else np.zeros(0, STATE_DTYPE), "means": means, "covs": covs, "best": best}


class Rig:
    """One map and the filters on it:
         mixed[0]  polar, stepped once (a max-likelihood state), a fitted three-component mixture; 300 particles (two workgroups)
         mixed[1]  Cartesian, before its first update, no mixture; 1 particle
         mixed[2]  polar, 0 particles
         twos      64 polar filters of 2 particles each, never updated"""

    def __init__(self, sc):
        import top_down_renderer_amd as pkg
        from top_down_renderer_amd import batch
        cfg = sc.cfg
        self.sc = sc
        self.m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
        self.m.sample_pts_polar(cfg.nb, cfg.nr, cfg.ang_res)
        self.m.set_window(8, 8)
        self.params = params = pkg.FilterParams(fixed_scale=1.0)
        self.r = batch.Renderer(sc.lut)
        self.r.render_polar(pcl(sc.pts), 8, 4, cfg.res, cfg.ang_res, cfg.ncls, cfg.nb, cfg.nr)
        f = batch.FilterHandle(self.m, 1024, params, seed=7)
        f.configure(1)
        f.set_states(sc.states)
        f.propagate(*MOTION)
        f.update(self.r, cfg.res)
        f.set_states(three_clumps(1024, 3))
        f.set_num_gaussians(2)
        f.compute_gmm()
        self.mixed = [f, batch.FilterHandle(self.m, 4, params, seed=8, cart=True), batch.FilterHandle(self.m, 4, params, seed=9)]
        self.twos = [batch.FilterHandle(self.m, 2, params, seed=20 + i) for i in range(64)]
        self.size = None

    def lay_out(self, H, W):
        """The map's background and every filter's particles for an H x W picture."""
        if self.size == (H, W):
            return self.bg
        self.bg = background(H, W, 100 + H)
        self.m.set_viz_background(self.bg)
        self.mixed[0].set_states(spread(300, H, W, 1))
        self.mixed[1].set_states(spread(1, H // 2, W // 2, 2))
        for i, f in enumerate(self.twos):
            f.set_states(spread(2, H, W, 10 + i))
        self.size = (H, W)
        return self.bg

    def fleet(self, k):
        """k filters: the mixed three at the highest indices where they fit, filters of 2 particles below them."""
        if k == 64:
            return self.twos
        return (self.twos[:max(k - 3, 0)] + self.mixed)[:k] if k >= 3 else self.mixed[:k]


@pytest.fixture(scope="module")
def L():
    from top_down_renderer_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene("c1", n_particles=512)


@pytest.fixture(scope="module")
def rig(scene):
    return Rig(scene)


def test_the_rig_is_what_the_tests_need(rig):
    rig.lay_out(37, 45)
    assert [f.num_particles() for f in rig.mixed] == [300, 1, 0] and all(f.num_particles() == 2 for f in rig.twos)
    rs = [robot(f) for f in rig.mixed]
    assert len(rs[0]["means"]) >= 2 and rs[0]["best"] is not None      # a mixture and a max-likelihood state
    assert len(rs[1]["means"]) == 0 and rs[1]["best"] is None and rig.mixed[1].cart


def check_fleet(rig, H, W, k, s, arrows, stream=None):
    from top_down_renderer_amd import batch
    bg = rig.lay_out(H, W)
    fs, pal = rig.fleet(k), palette(k)
    got = batch.visualize_fleet(fs, s, pal, arrows, stream=stream)
    want = FV.render([robot(f) for f in fs], bg, pal, arrows, s)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:5]
    return got


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("H,W", BACKGROUNDS)
def test_three_mixed_robots_equal_the_restatement(rig, H, W, s):
    """Polar beside Cartesian, after the first update beside before it, a mixture beside none, 300 / 1 / 0 particles."""
    got = check_fleet(rig, H, W, 3, s, [[2, 3, W - 3, H - 4], [W - 5, 5, W + 20, 9]])
    if s == 1.0:
        assert not np.array_equal(got, rig.bg)


@pytest.mark.parametrize("s", [1.0, 0.37])
@pytest.mark.parametrize("H,W", [(48, 64), (33, 130)])
@pytest.mark.parametrize("k", [1, 2, 33, 64])
def test_fleets_of_every_size_equal_the_restatement(rig, k, H, W, s):
    check_fleet(rig, H, W, k, s, None if k == 2 else [[1, 1, W - 2, H - 2]])


def test_fleet_picture_twice_and_on_a_stream(rig):
    import torch
    from top_down_renderer_amd import batch
    stream = torch.cuda.Stream()
    a = check_fleet(rig, 40, 144, 33, 0.5, [[5, 5, 100, 30]], stream=stream.cuda_stream)
    b = batch.visualize_fleet(rig.fleet(33), 0.5, palette(33), [[5, 5, 100, 30]])
    assert a.tobytes() == b.tobytes()


def test_identical_states_in_two_robots_show_the_higher_index(rig):
    from top_down_renderer_amd import batch
    H, W = 37, 45
    bg = rig.lay_out(H, W)
    fs = rig.twos[:3]
    st = spread(2, H // 2, W // 2, 77)
    st["dx_m"], st["dy_m"] = [3.0, -20.0], [2.0, 1.0]                  # one arrow inside, one dot
    fs[0].set_states(st)
    fs[1].set_states(st)
    fs[2].set_states(states_at(H, [(40, 30)], [0.3]))
    rig.size = None                                                    # (the next lay_out puts the states back)
    pal = palette(3)
    got = batch.visualize_fleet(fs, 1.0, pal)
    rs = [robot(f) for f in fs]
    assert np.array_equal(got, FV.render(rs, bg, pal))
    p0, p1, _ = FV.robot_planes(rs[1], H, W)
    assert p0.any() and p1.any() and not (p0 & p1).any()
    assert (got[p0] == pal[1, 0]).all() and (got[p1] == pal[1, 1]).all()   # robot 1's colours, none of robot 0's


def test_dot_arrow_and_ellipse_of_three_robots_on_the_same_pixels(rig):
    """The ellipse is robot 0's, the dot robot 1's, the arrow robot 2's: layer-major, so the lowest index shows."""
    from top_down_renderer_amd import batch
    H, W = 37, 45
    bg = rig.lay_out(H, W)
    f_est = rig.mixed[0]
    f_est.set_states(states_at(H, [(40, 5)], [0.0]))                   # its own particle far from the spot
    rig.size = None
    est = FV.robot_planes(robot(f_est), H, W)[2]
    ys, xs = np.nonzero(est[7:H - 7, 3:8])                             # estimate pixels a left dot can cover
    assert len(ys), "the mixture's ellipse does not cross the column of the left dots"
    x0, y0 = int(xs[0]) + 3, int(ys[0]) + 7
    f_dot, f_arrow = rig.twos[0], rig.twos[1]
    f_dot.set_states(states_at(H, [(-9, y0)], [0.0]))                  # clamped to (5, y0)
    f_arrow.set_states(states_at(H, [(x0, y0)], [1.0]))
    fs, pal = [f_est, f_dot, f_arrow], palette(3, 4)
    rs = [robot(f) for f in fs]
    planes = [FV.robot_planes(r, H, W) for r in rs]
    assert planes[0][2][y0, x0] and planes[1][1][y0, x0] and planes[2][0][y0, x0]
    got = batch.visualize_fleet(fs, 1.0, pal)
    assert np.array_equal(got, FV.render(rs, bg, pal))
    assert tuple(got[y0, x0]) == tuple(pal[0, 2])
    # the other way round the highest layer still wins: the ellipse robot last
    fs2 = [f_arrow, f_dot, f_est]
    got2 = batch.visualize_fleet(fs2, 1.0, pal)
    assert np.array_equal(got2, FV.render([rs[2], rs[1], rs[0]], bg, pal)) and tuple(got2[y0, x0]) == tuple(pal[2, 2])
    only_lower = batch.visualize_fleet([f_arrow, f_dot], 1.0, pal[:2])
    assert tuple(only_lower[y0, x0]) == tuple(pal[1, 1])               # dot over arrow


@pytest.mark.parametrize("s", [1.0, 0.5])
@pytest.mark.parametrize("H,W", [(37, 45), (48, 64)])
def test_one_robot_in_the_classic_colours_equals_filter_visualize(rig, H, W, s):
    from top_down_renderer_amd import batch
    bg = rig.lay_out(H, W)
    f = rig.mixed[0]
    f.set_viz_background(bg)                                           # its own copy of the same background
    arrows = [[2, 3, W - 3, H - 4]]
    got = batch.visualize_fleet([f], s, [batch.CLASSIC_PALETTE], arrows)
    assert np.array_equal(got, f.visualize(s, arrows))


def test_label_background_on_the_map(rig):
    from top_down_renderer_amd import batch
    H, W = 37, 45
    rig.lay_out(H, W)
    lab = np.random.default_rng(3).integers(0, 256, (H, W), dtype=np.uint8)
    lut = np.random.default_rng(4).integers(0, 256, (256, 3), dtype=np.uint8)
    rig.m.set_viz_background(labels=lab, lut=lut)
    rig.size = None
    fs, pal = rig.fleet(3), palette(3)
    got = batch.visualize_fleet(fs, 1.0, pal)
    assert np.array_equal(got, FV.render([robot(f) for f in fs], S.label_picture(lab, lut), pal))


def test_after_a_batched_step_and_filters_unchanged(scene):
    """Right after step_batch on an explicit stream the picture is of the stepped states; and pictures change nothing:
    filters that were drawn between two steps end on the bytes of twins that were not (states, weights, resample indices
    — which the generator's position decides)."""
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    sc, cfg = scene, scene.cfg
    H, W = sc.class_maps.shape[1:]
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, cfg.ang_res)
    bg = background(H, W, 5)
    m.set_viz_background(bg)
    params = pkg.FilterParams(fixed_scale=1.0)
    rng = np.random.default_rng(11)
    drawn, twins, rs = [], [], []
    for i in range(3):
        st = sc.states.copy()
        st["dx_m"] += rng.normal(0, 0.5, len(st)).astype(F32)
        for fl in (drawn, twins):
            f = batch.FilterHandle(m, len(st), params, seed=31 + i)
            f.configure(1)
            f.set_states(st)
            fl.append(f)
        r = batch.Renderer(sc.lut)
        r.render_polar(pcl(sc.pts[rng.random(len(sc.pts)) < 0.9]), 8, 4, cfg.res, cfg.ang_res, cfg.ncls, cfg.nb, cfg.nr)
        rs.append(r)
    stream = torch.cuda.Stream()
    pal = palette(3)
    batch.step_batch(drawn, rs, cfg.res, [MOTION] * 3, stream=stream.cuda_stream)
    got = batch.visualize_fleet(drawn, 0.5, pal, [[5, 5, 40, 20]], stream=stream.cuda_stream)
    robots = [robot(f) for f in drawn]
    assert all(r["best"] is not None for r in robots)
    assert np.array_equal(got, FV.render(robots, bg, pal, [[5, 5, 40, 20]], 0.5))
    before = [(f.states().tobytes(), f.weights().tobytes()) for f in drawn]
    batch.visualize_fleet(drawn, 1.0, pal)
    assert [(f.states().tobytes(), f.weights().tobytes()) for f in drawn] == before
    batch.step_batch(twins, rs, cfg.res, [MOTION] * 3)
    for fl in (drawn, twins):
        batch.step_batch(fl, rs, cfg.res, [MOTION] * 3)
    for f, t in zip(drawn, twins):
        assert f.states().tobytes() == t.states().tobytes() and f.weights().tobytes() == t.weights().tobytes()
        assert f.resample_indices().tobytes() == t.resample_indices().tobytes()


def test_refusals_leave_the_image_and_the_sizes_untouched(rig, scene, L):
    import test_viz as TV
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    H, W = 37, 45
    rig.lay_out(H, W)
    fs = rig.fleet(3)
    pal, s = palette(64), C.c_float(0.5)
    oh, ow = V.published_size(H, W, 0.5)
    out = np.full((oh, ow, 3), 0xA5, np.uint8)
    arrows = np.asarray([[1, 1, 20, 20]], np.int32)
    arr = (vp * 3)(*[f.h for f in fs])

    def refused(word, f=arr, k=3, scale=s, p=P(pal), a=P(arrows), m=1, cap=out.size):
        h, w = C.c_int(-7), C.c_int(-7)
        rc = L.tdr_batch_visualize_fleet(f, k, scale, p, a, m, P(out), cap, C.byref(h), C.byref(w), None)
        assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
        assert (out == 0xA5).all() and (h.value, w.value) == (-7, -7)

    refused("k = 0", k=0)
    refused("k = 65", f=(vp * 65)(*[g.h for g in rig.twos], fs[0].h), k=65)
    refused("null filter array", f=None)
    refused("filter 1 is null", f=(vp * 3)(fs[0].h, None, fs[2].h))
    refused("twice", f=(vp * 3)(fs[0].h, fs[1].h, fs[0].h))
    refused("null palette", p=None)
    refused("bad arrows", a=None)
    refused("bad arrows", m=-1)
    for bad, word in ((1e-4, "publishes 0 x 0"), (math.nan, "publishes"), (1e4, "publishes")):
        refused(word, scale=C.c_float(bad))
    refused("the image needs", cap=out.size - 1)
    # filters on different maps, a map without a background
    sc = scene
    other = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    other.sample_pts_polar(sc.cfg.nb, sc.cfg.nr, sc.cfg.ang_res)
    stranger = batch.FilterHandle(other, 4, rig.params, seed=3)
    refused("filter 2 is on another map", f=(vp * 3)(fs[0].h, fs[1].h, stranger.h))
    refused("the map has no background", f=(vp * 1)(stranger.h), k=1)
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
        refused("filter 1 is sharded", f=(vp * 3)(fs[0].h, hs.f, fs[2].h))
    finally:
        hs.close()
        L.tdr_comm_destroy(comm)
    # the setters and the launcher refuse before any device work too
    assert L.tdr_map_set_viz_background(rig.m.h, None, 20, 20) == -1
    assert L.tdr_map_set_viz_background(rig.m.h, P(out), 10, 20) == -1 and b"10 x 20" in L.tdr_last_error()
    assert L.tdr_map_set_viz_background_labels(rig.m.h, P(out), 20, 20, None) == -1
    assert L.tdr_map_set_viz_background_labels(rig.m.h, P(out), 20, 40000, P(out)) == -1
    d = vp(64)
    assert L.tdr_k_viz_compose_fleet(d, 0, P(pal), d, 20, 20, d, 20, 20, d, None) == -1 and b"k = 0" in L.tdr_last_error()
    assert L.tdr_k_viz_compose_fleet(d, 65, P(pal), d, 20, 20, d, 20, 20, d, None) == -1
    assert L.tdr_k_viz_compose_fleet(d, 2, None, d, 20, 20, d, 20, 20, d, None) == -1 and b"null" in L.tdr_last_error()
    assert L.tdr_k_viz_compose_fleet(d, 2, P(pal), d, 10, 20, d, 10, 20, d, None) == -1
    assert L.tdr_k_viz_compose_fleet(d, 2, P(pal), d, 20, 20, d, 0, 20, d, None) == -1
    assert L.tdr_k_viz_compose_fleet(d, 2, P(pal), d, 20, 20, None, 20, 20, d, None) == -1
    # and the fleet still draws: the size query sets the sizes and leaves the image alone
    h, w = C.c_int(-7), C.c_int(-7)
    assert L.tdr_batch_visualize_fleet(arr, 3, s, P(pal), None, 0, None, 0, C.byref(h), C.byref(w), None) == 0
    assert (h.value, w.value) == (oh, ow) and (out == 0xA5).all()
    assert L.tdr_batch_visualize_fleet(arr, 3, s, P(pal), P(arrows), 1, P(out), out.size, C.byref(h), C.byref(w), None) == 0
    assert np.array_equal(out, FV.render([robot(f) for f in fs], rig.bg, pal[:3], arrows, 0.5))


def test_a_filter_without_its_own_background_is_still_refused(rig):
    """The map's background is the fleet picture's: tdr_filter_visualize and tdr_batch_visualize keep asking for the
    filter's own."""
    from top_down_renderer_amd import batch
    from top_down_renderer_amd._lib import TdrError
    rig.lay_out(37, 45)
    bare = batch.FilterHandle(rig.m, 4, rig.params, seed=5)
    bare.set_states(spread(4, 37, 45, 1))
    with pytest.raises(TdrError, match="no background"):
        bare.visualize(1.0)
    with pytest.raises(TdrError, match="has no background"):
        batch.visualize_batch([bare], 1.0)
    assert batch.visualize_fleet([bare], 1.0, [batch.CLASSIC_PALETTE]).shape == (37, 45, 3)


@pytest.mark.parametrize("s", [1.0, 0.37])
@pytest.mark.parametrize("H,W", [(48, 64), (33, 130)])
def test_launcher_on_torch_buffers_equals_the_handle_call(rig, H, W, s):
    import torch
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.kernels import HipKernels, viz_overlay_host
    k = HipKernels()
    bg = rig.lay_out(H, W)
    fs, pal, arrows = rig.fleet(5), palette(5), [[3, 3, W - 4, H - 4]]
    robots = []
    for f in fs:
        r = robot(f)
        n = len(r["st"])
        dev = k.zeros((7, max(n, 1)))
        if n:
            k.states_to_device(r["st"], dev, n)
        segs = viz_overlay_host(r["means"], r["covs"], None, None, H)
        robots.append((dev, n, segs, None if r["best"] is None else k.to_device(np.asarray(r["best"], F32))))
    oh, ow = V.published_size(H, W, s)
    out = k.viz_draw_fleet(robots, k.to_device(bg), pal, arrows, oh, ow)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), batch.visualize_fleet(fs, s, pal, arrows))


def test_loop_batch_fleet_picture(scene):
    """LoopBatch.fleet_picture after a take_step: the picture of the loop's filters."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.top_down_render_core import CoreConfig
    sc, cfg = scene, scene.cfg
    H, W = sc.class_maps.shape[1:]
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, cfg.ang_res)
    bg = background(H, W, 6)
    m.set_viz_background(bg)
    fs = []
    for i in range(2):
        f = batch.FilterHandle(m, len(sc.states), pkg.FilterParams(fixed_scale=1.0), seed=41 + i)
        f.configure(1)
        f.set_states(sc.states)
        fs.append(f)
    loop = batch.LoopBatch(fs, [batch.Renderer(sc.lut) for _ in fs], CoreConfig(theta_bins=cfg.nb, range_bins=cfg.nr),
                           cfg.ang_res, cfg.ncls, cfg.nb, cfg.nr)
    loop.take_step([(pcl(sc.pts), 8, 4)] * 2, [MOTION] * 2)
    pal = palette(2)
    got = loop.fleet_picture(0.5, pal, [[5, 5, 40, 20]])
    assert np.array_equal(got, FV.render([robot(f) for f in fs], bg, pal, [[5, 5, 40, 20]], 0.5))


# ---- the C++ classes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade_fleet_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_fleet")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_fleet.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip",
                    f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def test_cpp_classes_draw_the_fleet_picture(scene, facade_fleet_exe):
    """TopDownMap::setVizBackground, TopDownRenderCoreBatch::renderFleetPicture and ParticleFilterBatch::renderFleet after
    one batched step of three robots: the image the program writes back equals the restatement on the states, mixtures
    and max-likelihood states it writes beside it; a second image over a label background likewise."""
    sc, cfg = scene, scene.cfg
    ncls, rows, cols = sc.class_maps.shape
    nb, nr = cfg.nb, cfg.nr
    pub_scale = 0.5
    d = tempfile.mkdtemp(prefix="tdr_fleet_")
    rng = np.random.default_rng(17)
    bg = background(rows, cols, 60)
    lab = rng.integers(0, 256, (40, 144), dtype=np.uint8)
    packed = rng.integers(0, 1 << 24, 256).astype(np.uint32)
    lut = np.stack([(packed >> 16) & 255, (packed >> 8) & 255, packed & 255], axis=1).astype(np.uint8)   # unpackColor as {B, G, R}
    pal = palette(3, 9)
    arrows = np.asarray([[5, 5, 40, 20], [cols - 4, 3, cols + 9, 8]], np.int32)
    open(os.path.join(d, "meta.txt"), "w").write(f"{ncls} {rows} {cols} {nb} {nr} {pub_scale} {rows} {cols} 40 144\n")
    np.ascontiguousarray(np.transpose(sc.class_maps, (0, 2, 1)), F32).tofile(os.path.join(d, "maps.bin"))
    np.ascontiguousarray(sc.class_mask.T, np.uint8).tofile(os.path.join(d, "mask.bin"))
    packed.tofile(os.path.join(d, "lut.bin"))
    bg.tofile(os.path.join(d, "bg.bin"))
    lab.tofile(os.path.join(d, "labels.bin"))
    pal.tofile(os.path.join(d, "palette.bin"))
    arrows.tofile(os.path.join(d, "arrows.bin"))
    for r in range(3):
        st = sc.states.copy()
        st["dx_m"] += rng.normal(0, 0.5, len(st)).astype(F32)
        st.tofile(os.path.join(d, f"states_{r}.bin"))
        pcl(sc.pts[rng.random(len(sc.pts)) < 0.9]).tofile(os.path.join(d, f"pts_{r}.bin"))
    out = subprocess.run([facade_fleet_exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["ok", "3"], out.stdout

    def rd(name, dtype):
        return np.fromfile(os.path.join(d, name), dtype)

    robots = []
    for r in range(3):
        gmm = rd(f"out_gmm_{r}.bin", F32)
        kk = len(gmm) // 12
        robots.append({"st": rd(f"out_states_{r}.bin", STATE_DTYPE), "best": rd(f"out_best_{r}.bin", F32)[:3],
                       "means": gmm[:3 * kk].reshape(kk, 3), "covs": gmm[3 * kk:].reshape(kk, 3, 3)})
    assert len(robots[0]["means"]) >= 1                                # robot 0 has a fitted mixture
    for name, back, arr in (("out_fleet", bg, arrows), ("out_fleet_labels", S.label_picture(lab, lut), None)):
        want = FV.render(robots, back, pal, arr, pub_scale)
        h, w = rd(name + "_size.bin", np.int32)
        assert (h, w) == want.shape[:2], name
        assert np.array_equal(rd(name + ".bin", np.uint8).reshape(h, w, 3), want), name
