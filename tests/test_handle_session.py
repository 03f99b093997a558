"""One map, one renderer and one filter handle living through a whole scripted session, the CPU oracle in lock step
(tests/session_ref.py checks every call stage by stage on inputs read back from the device).

What the rest of the suite leaves open: the handle layer (csrc/tdr_host*.cpp) keeps some forty device buffers that only
grow and some ten remembered facts about their content (maybe_uninit, uniform_scale, scale_frozen, the cached pose, where
the random stream lives, the tuner, the map's scratch).  A kernel that is right on a fresh buffer can be wrong on one an
earlier, larger or differently shaped call left behind; a flag one entry point forgets turns a right kernel into a wrong
pose.  So here the particle count walks down into buffers that were larger and up again across every switch of the code
(4096 / 4097: the pose statistics; 32 768 / 32 769: the weight statistics and the one-launch running sum; 8192: the
half-record scratch of the heading search; 2304 = 64 x 36 rows: float against integer form), `res` changes every step, the
window shape, the scan source, the scale's state, the map (four entry points, one of them another size, resolution and
class count) and the process-wide switches change between steps.

Every script is a table of events (`SCRIPTS`); `test_scripts_are_worth_running` runs A, C and D on the oracle alone and
asserts that the inputs exercise what they are meant to.  Shapes are the smallest at which each path still runs."""
import numpy as np
import pytest

import session_ref as S

F32 = np.float32
N_MAX = 40_000
N_CART = 6000        # the Cartesian session: enough to stand on both sides of 4096 (the oracle scores 40 headings apiece)
MOTION = (0.3, 0.1, 0.01)
CW = [1.0, 0.5, 2.0, 1.5, 0.25, 1.0]
WALK = (3000, 40_000, 32_769, 32_768, 4097, 4096, 500, 1, 5000, 8193, 8192, 8191, 2305, 2304, 2303, 6000)


def _res(k):
    return 0.8 + 0.05 * (k % 9)      # another `res` on every step


# ---- the maps and clouds ---------------------------------------------------------------------------------------------
class World:
    """The first map (180 x 200 cells, 6 classes), variants of it for the map updates, the second map (150 x 170 cells,
    4 classes, resolution 0.5) and a cloud for each; made once."""
    _made = None

    @classmethod
    def get(cls, oracle):
        if cls._made is None:
            cls._made = cls(oracle)
        return cls._made

    def __init__(self, oracle):
        from oracle import np_oracle as no
        from top_down_renderer_amd import synth
        cfg = synth.Config("hs1", 3000, 6, 36, 12, 200, 16, seed=4242, res=1.0)
        sc = synth.make_scene(cfg, with_particles=False)
        lab = sc.lab[:180, :200]
        self.pose = sc.pose
        self.lut = synth.make_lut(6)
        img = np.where(lab >= 0, lab, 200).astype(np.uint8)[::-1].copy()        # cv::Mat layout, 200 = unlabelled
        maps, mask = no.load_compressed_raster_map(img, self.lut, 6, 1.0)
        self.m1 = S.MapSpec(maps, mask, 1.0, (0, 0), pts=sc.pts)
        # the same ground with a block relabelled, as distance maps, the centre moved
        img_b = img.copy()
        img_b[40:70, 30:80] = 3
        maps_b, mask_b = no.load_compressed_raster_map(img_b, self.lut, 6, 1.0)
        self.m1b = S.MapSpec(maps_b, mask_b, 1.0, (3, -2), pts=sc.pts)
        # the second map: another size, resolution and class count, from a label image
        rng = np.random.default_rng(77)
        lab2 = synth.make_label_image(100, 4, rng)[:75, :85]
        img2 = np.where(lab2 >= 0, lab2, 200).astype(np.uint8)[::-1].copy()
        cfg2 = synth.Config("hs2", 2500, 4, 36, 12, 170, 16, seed=78, res=1.0)
        cells = np.kron(lab2, np.ones((2, 2), np.int8))
        pts2 = synth.make_scan(cfg2, cells, (2 * (self.pose[0] - 52), 2 * (self.pose[1] - 90), 0.4), rng, scale=2.0)
        pts2[:, 3][pts2[:, 3] >= 4] = 200       # the renderer's table is the 6-class one: no raw id 4 or 5 in this cloud
        # (0.5 m cells: the map spans 85 x 75 px; the centre's move of (-52, -90) carries the particles onto it)
        self.m2 = S.labels_spec(no, img2, self.lut, 4, 0.5, (-49, -92), pts2)
        img3 = img2.copy()
        img3[20:26, 30:41] = 2
        img3[50:52, 60:70] = 1
        self.m2b = S.labels_spec(no, img3, self.lut, 4, 0.5, (-46, -95), pts2)
        img4 = img3.copy()
        self.patch = (33, 12, 9, 14)            # y0, x0, h, w in image pixels
        img4[33:42, 12:26] = 0
        self.m2c = S.labels_spec(no, img4, self.lut, 4, 0.5, (-50, -93), pts2)
        # Cartesian: the first map with a cloud rendered for a window
        cfgc = synth.Config("hsc", 3000, 6, 48, 64, 200, 16, polar=False, seed=4243, res=0.75)
        self.pts_c = synth.make_scan(cfgc, lab, self.pose, np.random.default_rng(5))
        self.m1c = S.MapSpec(maps, mask, 1.0, (0, 0), pts=self.pts_c)
        self.m1bc = S.MapSpec(maps_b, mask_b, 1.0, (3, -2), pts=self.pts_c)

    def params(self, **kw):
        p = dict(fixed_scale=-1.0, init_pos_px_x=float(self.pose[0]), init_pos_px_y=float(self.pose[1]), init_pos_px_cov=15.0,
                 init_pos_deg_theta=float("inf"), class_weights=CW)
        p.update(kw)
        return p


def _cloud(world, n, seed, kind):
    """States for set_states, around the pose the clouds were rendered from."""
    from top_down_renderer_amd import synth
    rng = np.random.default_rng(seed)
    st = np.zeros(n, synth.STATE_DTYPE)
    st["init_x_px"] = rng.normal(world.pose[0], 12, n)
    st["init_y_px"] = rng.normal(world.pose[1], 12, n)
    st["dx_m"], st["dy_m"] = rng.normal(0, 1, n), rng.normal(0, 1, n)
    st["theta"] = rng.uniform(-np.pi, np.pi, n)
    st["have_init"] = 1
    st["scale"] = F32(1.25)
    if kind == "unequal":
        st["scale"] = rng.uniform(0.8, 2.5, n)
    elif kind == "tenth":
        un = rng.random(n) < 0.15
        st["have_init"][un] = 0
        st["theta"][un] = 0
    elif kind == "offmap":
        st["init_x_px"][1:] += 5000
    return st


# ---- the scripts: tables of events ---------------------------------------------------------------------------------------
# ("step", n_target, {source, zero, geo, degenerate}) = propagate + update + pose at the next `res`; everything else is an
# event between steps.  Filter "a" unless the event names another.
def script_a():
    ev = [("init", "device"), ("step", WALK[0], dict(search=True))]
    for k, n in enumerate(WALK[1:]):                  # the walk: down into buffers that were larger, and up again
        ev.append(("step", n, dict(source="renderer" if k % 2 == 0 else "host")))
        if n == 4097:
            ev.append(("window", (25, 16)))
        if n == 8192:
            ev.append(("window", (36, 12)))
    ev += [
        ("reads",), ("step", -1, {}),
        ("freeze",), ("step", -1, dict(source="renderer")),                      # the uniform-scale table path
        ("set_states", "unequal", 5000), ("step", -1, {}),                       # uniform_scale must drop
        ("set_states", "equal", 5000), ("propagate_freeze", 0), ("compute_weights",), ("step", -1, {}),
        ("step", -1, dict(geo=True)), ("step", 4500, dict(source="renderer")), ("step", -1, dict(geo=True)),
        ("set_states", "tenth", 9000), ("step", 5000, dict(search=True)),        # the search runs again
        ("step", -1, dict(zero=True, degenerate=True)), ("step", -1, {}),        # an all-zero scan
        # all but one particle off the map: the oracle's weights are NaN but one and its resample keeps every particle, so
        # the step after it (which must be clean: every stage check holds) scores the same set; then a fresh cloud
        ("set_states", "offmap", 4100), ("step", -1, dict(degenerate=True)), ("step", 4096, dict(source="renderer", stuck=True)),
        ("set_states", "equal", 4096), ("step", -1, {}),
        ("init", "device"), ("step", 33_000, dict(search=True)),                 # in mid-run, on a frozen filter
        ("init", "host"), ("step", 3000, dict(search=True, source="renderer")),
        ("map", "maps", "m1b"), ("step", -1, {}),
        ("map", "labels", "m2"), ("step", -1, dict(source="renderer")), ("step", -1, dict(geo=True)),
        ("map", "incremental", "m2b"), ("step", -1, {}),
        ("map", "patch", "m2c"), ("step", 6000, dict(source="renderer")),
        ("configure", 0, 1), ("propagate",), ("configure", 1, 1), ("update", -1, {}), ("step", -1, {}),
    ]
    return ev


def script_b():
    """Process-wide switches flipped between the steps of one filter: the integer and the float form lay out the
    workspace differently, the compact and the dense records, the half-record search, the generator's stretches."""
    ALL_RAY = 1e-6
    ev = [("init", "device"), ("step", 20_000, dict(search=True))]
    flips = [[("shift_uniform", 2), ("span", 0.0)], [("shift_uniform", 0)], [("shift_uniform", 2), ("span", ALL_RAY)],
             [("compact", 0)], [("shift_uniform", 0), ("compact", 1), ("mt_stretches", 0)], [("shift_uniform", 2), ("span", -2.0)],
             [("rec16_min", 0), ("locality", 0)], [("shift_uniform", 0), ("mt_stretches", 1)],
             [("shift_uniform", 2), ("locality", 1), ("compact", 0)], [("compact", 1), ("span", 0.0)]]
    walk = (4097, 4096, 20_000, 2000, 9000, 4096, 12_000, 3000, 4097, 5000)
    for k, (fl, n) in enumerate(zip(flips, walk)):
        ev += [("switch",) + f for f in fl]
        if k in (3, 6, 8):
            ev.append(("set_states", "tenth", 9000 if k != 6 else 3000))
        ev.append(("step", n, dict(source="renderer" if k % 2 else "host", search=k in (3, 6, 8))))
    return ev


def script_c():
    return [
        ("init", "device"), ("step", 4097, dict(search=True)),                   # the cold-start heading search
        ("step", 4096, dict(source="renderer")), ("window", (36, 20)), ("step", 4095, {}),
        ("step", 4097, dict(source="renderer")), ("switch", "cart_seg_rows", 0), ("step", 4500, {}),
        ("window", (48, 64)), ("step", -1, dict(source="renderer")), ("switch", "cart_seg_rows", 32),
        ("set_states", "tenth", 4200), ("step", -1, dict(search=True)),
        ("reads",), ("map", "maps", "m1bc"), ("step", 600, dict(source="renderer")), ("step", 4097, {}),
        ("freeze",), ("step", -1, {}),
    ]


def script_d():
    """Two filters on one map and one renderer, stepping alternately: "a" polar, "b" Cartesian on the same tdr_map."""
    ev = [("switch", "rec16_min", 0), ("init", "device", "a"), ("init", "device", "b")]
    for k, (na, nb) in enumerate(((2000, 1500), (-1, 1200), (2500, -1))):
        if k == 1:
            ev += [("set_states", "tenth", 2000, "a"), ("set_states", "tenth", 1500, "b")]
        src = "renderer" if k != 1 else "host"
        ev += [("step", na, dict(source=src, search=k < 2), "a"), ("step", nb, dict(source=src, search=k < 2), "b")]
    return ev


SCRIPTS = {"A": script_a, "B": script_b, "C": script_c, "D": script_d}
SWITCHES = {
    "shift_uniform": lambda L, v: L.tdr_config_shift_uniform(int(v)),
    "span": lambda L, v: L.tdr_config_shift_uniform_span(float(v)),
    "compact": lambda L, v: L.tdr_config_compact(int(v)),
    "rec16_min": lambda L, v: L.tdr_config_rec16_min_particles(int(v)),
    "mt_stretches": lambda L, v: L.tdr_config_tuning(b"mt_stretches", int(v)),
    "cart_seg_rows": lambda L, v: L.tdr_config_tuning(b"cart_seg_rows", int(v)),
    "init_device": lambda L, v: L.tdr_config_tuning(b"init_device", int(v)),
}


def _sessions(oracle, name, handle):
    w = World.get(oracle)
    if name in ("A", "B"):
        return w, {"a": S.Session(oracle, w.m1, N_MAX, 23, w.params(), handle=handle, name=name)}
    if name == "C":
        return w, {"a": S.Session(oracle, w.m1c, N_CART, 29, w.params(), cart=True, shape=(48, 64), handle=handle, name=name)}
    a = S.Session(oracle, w.m1, 3000, 31, w.params(), handle=handle, name="D.a")
    b = S.Session(oracle, w.m1c, 2000, 37, w.params(class_weights=CW[::-1], init_pos_px_cov=9.0), cart=True, shape=(48, 64),
                  handle=handle, map_handle=a.map_handle, renderer=a.renderer, name="D.b")
    return w, {"a": a, "b": b}          # (the shared map carries both the polar table and the window)


def run(oracle, name, handle):
    """Runs script `name`; returns the sessions.  Process-wide switches are put back whatever happens."""
    w, ses = _sessions(oracle, name, handle)
    L, saved, k = None, {}, 0
    if handle:
        from top_down_renderer_amd import _lib
        L = _lib.load()
        saved = {"shift_uniform": L.tdr_config_shift_uniform(-1), "compact": L.tdr_config_compact(-1),
                 "rec16_min": L.tdr_config_rec16_min_particles(-1), "mt_stretches": L.tdr_config_tuning(b"mt_stretches", -1),
                 "cart_seg_rows": L.tdr_config_tuning(b"cart_seg_rows", -1), "init_device": L.tdr_config_tuning(b"init_device", -1)}
    try:
        for i, e in enumerate(SCRIPTS[name]()):
            kind = e[0]
            who = e[-1] if isinstance(e[-1], str) and e[-1] in ses and kind in ("init", "set_states", "step") else "a"
            s = ses[who]
            tag = f"#{i} {e}"
            if kind == "init":
                if L:
                    SWITCHES["init_device"](L, 1 if e[1] == "device" else 0)
                s.initialize(tag)
            elif kind in ("step", "update"):
                opt = {kk: v for kk, v in e[2].items() if kk not in ("search", "stuck")}
                if kind == "step":
                    s.propagate(*MOTION)
                s.update(_res(k), e[1], **opt)
                s.records[-1].update(event=i, want_search=bool(e[2].get("search")), stuck=bool(e[2].get("stuck")))
                s.label = tag
                k += 1
            elif kind == "propagate":
                s.propagate(*MOTION, label=tag)
            elif kind == "propagate_freeze":
                s.propagate(*MOTION, freeze=e[1], label=tag)
            elif kind == "compute_weights":
                s.compute_weights(_res(k), label=tag)
            elif kind == "set_states":
                s.set_states(_cloud(w, e[2], 100 + i, e[1]), tag)
            elif kind == "freeze":
                s.freeze(tag)
            elif kind == "window":
                s.window(e[1], tag)
            elif kind == "reads":
                s.reads(tag)
            elif kind == "configure":
                s.configure(e[1], e[2], tag)
            elif kind == "map":
                changed = s.new_map(getattr(w, e[2]), e[1], tag, patch=w.patch if e[1] == "patch" else None)
                # (on a map this small every changed cell lies within the distance cap of most of the map: the incremental
                # call reports -1, its own full path; the patch has no such limit and reports the cells it rebuilt)
                if handle and e[1] == "patch":
                    assert changed > 0, (tag, changed)
                if handle and e[1] == "incremental":
                    assert changed != 0, (tag, changed)
            elif kind == "switch":
                if e[1] == "locality":
                    s.configure(1, e[2], tag)
                elif L:
                    SWITCHES[e[1]](L, e[2])
            else:
                raise AssertionError(f"unknown event {e}")
    finally:
        if L:
            for key, v in saved.items():
                SWITCHES[key](L, v)
            L.tdr_config_shift_uniform_span(-2.0)
    return ses


# ---- the scripts on the oracle alone ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dry(oracle):
    return {name: run(oracle, name, handle=False) for name in ("A", "C", "D")}


def test_scripts_are_worth_running(oracle, dry):
    """Conditions on the INPUTS, met by the oracle alone: every kind of event occurs and is followed by a scored step, the
    walk holds the listed counts, the weights of every step but the two designated degenerate ones are mostly finite and
    non-zero and its resample keeps many sources, and the search steps do search."""
    ev = script_a()
    kinds = {e[0] for e in ev}
    assert kinds >= {"init", "step", "window", "reads", "freeze", "set_states", "propagate_freeze", "compute_weights", "map",
                     "configure", "propagate", "update"}
    assert {e[1] for e in ev if e[0] == "set_states"} == {"unequal", "equal", "tenth", "offmap"}
    assert {e[1] for e in ev if e[0] == "map"} == {"maps", "labels", "incremental", "patch"}
    assert {e[1] for e in ev if e[0] == "init"} == {"device", "host"}
    steps = [e for e in ev if e[0] == "step"]
    assert {e[2].get("source", "host") for e in steps} == {"host", "renderer"}
    assert any(e[2].get("geo") for e in steps) and any(e[2].get("zero") for e in steps)
    assert sum(bool(e[2].get("degenerate")) for e in steps) == 2
    ia = [i for i, e in enumerate(ev) if e == ("set_states", "equal", 5000)][0]
    assert [e[0] for e in ev[ia:ia + 4]] == ["set_states", "propagate_freeze", "compute_weights", "step"] and ev[ia + 1][1] == 0
    for name in ("A", "C", "D"):
        table = SCRIPTS[name]()
        assert table[-1][0] == "step"
        for i, e in enumerate(table):                         # every event is followed by a scored step, soon
            if e[0] not in ("step", "update"):
                assert any(x[0] in ("step", "update") for x in table[i + 1:i + 5]), (name, e)
    ra = dry["A"]["a"].records
    ns = [r["n"] for r in ra] + [ra[-1]["n_new"]]
    for a, b in zip((N_MAX,) + WALK, WALK):                   # the walk, in order: each count is scored and left
        assert any(r["n"] == a and r["n_new"] == b for r in ra), (a, b)
    for want in (3000, 40_000, 32_769, 32_768, 4097, 4096, 500, 1, 5000):
        assert want in ns
    assert len({r["res"] for r in ra}) >= 9 and all(x["res"] != y["res"] for x, y in zip(ra, ra[1:]))
    assert {r["shape"] for r in ra} == {(36, 12), (25, 16)} and {r["ncls"] for r in ra} == {6, 4}
    ic = [i for i, e in enumerate(ev) if e[0] == "configure"]          # one propagate on the device's own generator
    assert [ev[i][1] for i in ic] == [0, 1]
    assert [e[0] for e in ev[ic[0]:ic[1] + 2]] == ["configure", "propagate", "configure", "update"]
    for name, who in (("A", "a"), ("C", "a"), ("D", "a"), ("D", "b")):
        rec = dry[name][who].records
        assert sum(r["degenerate"] for r in rec) == (2 if name == "A" else 0) and sum(r["stuck"] for r in rec) == (name == "A")
        for r in rec:
            tag = (name, who, r["label"], r)
            if r["stuck"]:      # the step after the off-map one: the oracle's resample left the set as it was
                assert r["good"] <= 0.5 and r["n"] == 4100 and rec[rec.index(r) - 1]["distinct"] == 4100, tag
            elif not r["degenerate"]:
                assert r["good"] > 0.5, tag
                if r["n"] >= 20 and r["n_new"] >= 20:
                    assert r["distinct"] >= r["n_new"] / 20, tag
            if r["want_search"]:
                assert r["search"] >= 0.1, tag
        assert any(r["want_search"] for r in rec)
    rc = dry["C"]["a"].records
    assert {r["shape"] for r in rc} == {(48, 64), (36, 20)} and {r["source"] for r in rc} == {"host", "renderer"}
    nc = {r["n"] for r in rc}
    assert {4095, 4096, 4097} <= nc
    assert dry["D"]["a"].cart is False and dry["D"]["b"].cart is True


# ---- the sessions on the GPU -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_session_a_polar_unknown_scale(oracle):
    """Script A: a polar filter on the parity generator with an unknown scale — the particle-count walk, both scan sources,
    both window shapes, freeze_scale, set_states of every kind, propagate_freeze(0) on a filter that promised a uniform
    scale, an all-zero scan, a step with all but one particle off the map, update_geo interleaved, the map replaced through
    each of the four entry points (one of them 6 -> 4 classes at another size and resolution), initialize_particles in
    mid-run on the device and on the host, one propagate on the device's own generator."""
    run(oracle, "A", handle=True)


@pytest.mark.gpu
def test_session_b_switches_flip_between_steps(oracle):
    """Script B: the same filter while the process-wide switches flip between steps (integer / float form on one
    workspace, span 0 / all-ray / tuned, compact records, the half-record search, the generator's stretches, locality)."""
    run(oracle, "B", handle=True)


@pytest.mark.gpu
def test_session_c_cartesian(oracle):
    """Script C: a Cartesian handle — cold-start search, the other window between updates, the walk across 4096, both scan
    sources, un-initialised particles again, cart_seg_rows 0 / 32, a map replacement, freeze_scale."""
    run(oracle, "C", handle=True)


@pytest.mark.gpu
def test_session_d_two_filters_share_a_map(oracle):
    """Script D: a polar and a Cartesian filter on ONE tdr_map and one renderer, stepping alternately, each with its own
    class weights, count, seed and oracle; both search, on half records (the map's scratch holds the searching filter's
    class weights).  The centre does not move here: what a second filter should do once the first has moved a shared
    map's centre is a question of the contract, not of this test."""
    run(oracle, "D", handle=True)
