"""tdr_k_score_cart_init (csrc/tdr_score_cart_init.hip): the heading search of the Cartesian filter, as a launcher.

For a particle without a heading the search takes the first of the reference's 40 candidate headings (the float loop
of src/state_particle.cpp:197) whose Cartesian cost is strictly smaller than all earlier ones, NaN never chosen; theta = 0
when no candidate is finite; have_init = 1 afterwards; nothing else changes.  Expected values come from the CPU oracle:
every candidate of every particle scored by oracle.compute_weights_cart, the first maximum of the weight with NaN skipped.
A different device choice passes only if the oracle rates it within 2e-5 (relative) of its own maximum — the tie rule and
the number of test_init_search_c1; every mismatch is checked, there is no floor on agreement.  Weights at the chosen
heading: within 1e-5 of the oracle (the project's Cartesian tolerance)."""
import ctypes as C

import numpy as np
import pytest
from cart_ref import CASES, candidates, check_search, make_case, oracle_candidate_weights

from top_down_renderer_amd import synth


# ---- CPU: arguments ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from top_down_renderer_amd import _lib, build
    build.build()
    return _lib.load()


def test_candidates_are_the_forty_of_the_float_loop():
    th = candidates()
    assert len(th) == 40 and th[0] == 0 and th[-1] < 2 * np.pi
    assert th[1] == np.float32(2 * np.pi / 40)


def test_argument_errors_come_before_any_device_work(lib):
    """No device is needed to be told that an argument is wrong (the convention of tdr_k_score_cart)."""
    from top_down_renderer_amd import _lib
    desc = _lib.MapDescC()
    desc.rec, desc.ncls, desc.rows, desc.cols, desc.rec_floats, desc.resolution = 8, 6, 300, 260, 8, 1.0
    fp = _lib.FilterParamsC()
    fp.num_classes = 6
    d = C.c_void_p(8)
    one = C.c_float(1.0)

    def call(map_=C.byref(desc), scan=d, rows=32, cols=24, st=d, cap=10, n=10, ws=d):
        return lib.tdr_k_score_cart_init(map_, scan, rows, cols, one, C.byref(fp), st, cap, n, 0, ws, None)

    for kw in (dict(map_=None), dict(scan=None), dict(st=None), dict(ws=None), dict(rows=0), dict(cols=0), dict(n=-1),
               dict(n=11)):
        assert call(**kw) == -1, kw
        assert b"score_cart_init" in lib.tdr_last_error()
    nomap = _lib.MapDescC()
    assert call(map_=C.byref(nomap)) == -1      # a descriptor without records
    assert call(n=0) == 0                       # nothing to do is not an error, and launches nothing


def test_chunk_knob_bounds_the_workspace(lib):
    before = lib.tdr_config_tuning(b"cart_init_chunk", -1)
    assert before >= 1
    try:
        sizes = {}
        for chunk in (16, 1024):
            assert lib.tdr_config_tuning(b"cart_init_chunk", chunk) == chunk
            sizes[chunk] = lib.tdr_score_cart_init_workspace_floats(6, 32, 24, 100000, 100000)
        # list + per chunk: 40 candidates x (7 state planes + 1 weight) + the scoring launch's own workspace for them
        for chunk, floats in sizes.items():
            assert floats >= 100000 + 40 * chunk * 8 + lib.tdr_score_cart_workspace_floats(6, 32, 24, 40 * chunk, 100000)
        assert sizes[16] < sizes[1024]
        # a filter smaller than the chunk pays for its own particles only
        assert lib.tdr_score_cart_init_workspace_floats(6, 32, 24, 8, 8) < sizes[16]
    finally:
        lib.tdr_config_tuning(b"cart_init_chunk", before)
    assert lib.tdr_config_tuning(b"cart_init_chunk", -1) == before


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tdr():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pkg, HipKernels()


@pytest.fixture(scope="module")
def scenes(tdr, oracle):
    """Per case: the device map and packed scan, the oracle's map / scan / parameters and its (N_ALL, 40) candidate
    weights — computed once, shared, never modified."""
    pkg, k = tdr
    out = {}
    for name, (ncls, rows, cols, _) in CASES.items():
        cfg, lab, maps, mask, pose, pts, st = make_case(name)
        om = oracle.OracleMap(maps, mask, 1.0)
        scan = oracle.raster_cart(pts, cfg.res, synth.make_lut(ncls), ncls, rows, cols)
        cw = [float(0.5 + (c % 4) * 0.5) for c in range(ncls)]
        fpo = oracle.make_params(ncls, class_weights=cw)
        m = pkg.TopDownMap(pkg.Params(resolution=1.0), maps, mask, kernels=k)
        m.setWindow(rows, cols)
        w40 = oracle_candidate_weights(oracle, om, rows, cols, scan, cfg.res, fpo, st)
        w40.setflags(write=False)
        st.setflags(write=False)
        out[name] = dict(cfg=cfg, om=om, scan=scan, fpo=fpo, m=m, pk=m.scan_handle(np.ascontiguousarray(scan)),
                         fp=pkg.FilterParams(fixed_scale=1.0, class_weights=cw).to_c(ncls), st=st, w40=w40, pose=pose)
    return out


def run_search(tdr, s, st, n_total=0):
    """tdr_k_score_cart_init + tdr_k_score_cart on a plane stride that is not the particle count."""
    pkg, k = tdr
    n = len(st)
    ncls, rows, cols = s["cfg"].ncls, s["cfg"].nb, s["cfg"].nr
    dev = k.zeros((7, n + 5))
    k.states_to_device(st, dev, n)
    raw = k.zeros((n + 5,))
    k.score_cart_init(s["m"].dev, s["pk"], rows, cols, s["cfg"].res, s["fp"], dev, n, n_total=n_total)
    k.score_cart(s["m"].dev, s["pk"], rows, cols, s["cfg"].res, s["fp"], dev, n, raw, n_total=n_total)
    k.synchronize()
    return k.states_to_host(dev, n, pkg.STATE_DTYPE), raw[:n].cpu().numpy()


def subset(s, first, n, mixed):
    st = s["st"][first:first + n].copy()
    st["have_init"] = 0
    st["theta"] = 0
    if mixed:   # every other particle already has a heading
        st["have_init"][1::2] = 1
        st["theta"][1::2] = np.random.default_rng(9).uniform(-np.pi, np.pi, len(st[1::2])).astype(np.float32)
    return st


@pytest.fixture
def form(tdr, request):
    """tdr_config_shift_uniform(mode) for the test, restored afterwards."""
    k = tdr[1]
    before = k.lib.tdr_config_shift_uniform(-1)
    k.lib.tdr_config_shift_uniform(request.param)
    yield request.param
    k.lib.tdr_config_shift_uniform(before)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 2], indirect=True)
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("first,n", [(0, 1), (7, 1), (0, 63), (0, 200)])
@pytest.mark.parametrize("case", list(CASES))
def test_search_matches_the_oracle(tdr, oracle, scenes, case, first, n, mixed, form):
    s = scenes[case]
    st = subset(s, first, n, mixed)
    got_st, got_raw = run_search(tdr, s, st)
    if first == 0:   # the far-off particle: no finite candidate -> theta 0 (the border particle [1]: checked like the rest)
        assert not np.isfinite(s["w40"][0]).any()
        assert got_st["theta"][0] == 0 and got_st["have_init"][0] == 1 and np.isnan(got_raw[0])
    check_search(oracle, s["om"], s["cfg"].nb, s["cfg"].nr, s["scan"], s["cfg"].res, s["fpo"], st,
                 s["w40"][first:first + n], got_st, got_raw)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 2], indirect=True)
@pytest.mark.parametrize("chunk", [1, 7])
@pytest.mark.parametrize("case", list(CASES))
def test_chunked_search_equals_the_unchunked_one(tdr, oracle, scenes, case, chunk, form):
    """63 particles in chunks of 1 and of 7 — nine whole chunks, or four and a ragged fifth over the 32 particles without
    a heading of the mixed set: the headings of the one-chunk run, or ties under the oracle's rule."""
    pkg, k = tdr
    s = scenes[case]
    before = k.tuning("cart_init_chunk")
    try:
        for mixed in (False, True):
            st = subset(s, 0, 63, mixed)
            k.tuning("cart_init_chunk", 4096)
            whole_st, whole_raw = run_search(tdr, s, st)
            k.tuning("cart_init_chunk", chunk)
            got_st, got_raw = run_search(tdr, s, st)
            same = got_st["theta"] == whole_st["theta"]
            print(f"chunk {chunk}, mixed {mixed}: {int(same.sum())} of {len(same)} headings equal the one-chunk run's")
            if same.all():
                assert np.array_equal(got_raw, whole_raw, equal_nan=True)
            check_search(oracle, s["om"], s["cfg"].nb, s["cfg"].nr, s["scan"], s["cfg"].res, s["fpo"], st, s["w40"][:63],
                         got_st, got_raw)
    finally:
        k.tuning("cart_init_chunk", before)


@pytest.mark.gpu
def test_scoring_launches_follow_the_number_of_particles_without_a_heading(tdr, scenes):
    """No particle without a heading: no scoring launch at all, and the states stay as they are.  32 of them in chunks of
    7: five scoring launches."""
    pkg, k = tdr
    s = scenes["c6_32x24"]
    cfg = s["cfg"]
    before = k.tuning("cart_init_chunk")
    k.lib.tdr_profile_enable(1)
    try:
        k.tuning("cart_init_chunk", 7)
        for mixed, want in ((None, 0), (True, 5), (False, 9)):
            st = subset(s, 0, 63, bool(mixed))
            if mixed is None:
                st["have_init"] = 1
                st["theta"] = np.linspace(-3, 3, len(st)).astype(np.float32)
            dev = k.zeros((7, 64))
            k.states_to_device(st, dev, len(st))
            ms, launches = C.c_double(0), C.c_int64(0)
            k.lib.tdr_profile_score_ms(C.byref(ms), C.byref(launches))   # reset
            k.score_cart_init(s["m"].dev, s["pk"], cfg.nb, cfg.nr, cfg.res, s["fp"], dev, len(st))
            k.lib.tdr_profile_score_ms(C.byref(ms), C.byref(launches))
            assert launches.value == want, (mixed, launches.value)
            if mixed is None:
                back = k.states_to_host(dev, len(st), pkg.STATE_DTYPE)
                for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "theta", "scale", "have_init"):
                    assert np.array_equal(back[name], st[name]), name
    finally:
        k.lib.tdr_profile_enable(0)
        k.tuning("cart_init_chunk", before)
