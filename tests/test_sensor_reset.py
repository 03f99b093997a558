"""GPU: sensor resetting (csrc/tdr_recover_sensor.hip, csrc/tdr_host_recover.cpp; include/tdr.h, "sensor resetting") against
its NumPy restatement (tests/sensor_reset_ref.py), with ==: the three kernels through their launchers, the handle against
the device's own scorer (a second filter of the same kind, map, parameters and particle count scores the restatement's
candidates), chunking, C = 1 against the plain injection, the CPU oracle's picks, what is refused, and what the feature is
for: one call on the kidnapped robot's scan puts particles into the basin that the uniform injection misses.
Sizes are chosen for where the kernels can go wrong (a lane, a wave less one, a wave, a wave plus one, several workgroups
with a ragged end, a grid smaller than the tiles), not for the workload."""
import ctypes as C

import numpy as np
import pytest

import recovery_ref as RR
import sensor_reset_ref as SR
from test_recovery import _dev_map, _handle, _road_maps, _snapshot, _spread_states, _states, _to_planes

pytestmark = pytest.mark.gpu
F32 = np.float32
vp = C.c_void_p
FULL = 1 << 24
NAN = float("nan")
SENT = -777.0


@pytest.fixture(scope="module")
def K():
    import torch
    from top_down_renderer_amd.kernels import HipKernels
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def _planes_of(states):
    """(7, n) float32 planes of a STATE_DTYPE array."""
    return _to_planes(np.ascontiguousarray(states).reshape(-1), states.size, 0.0)


# ---- the list kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_list_equals_the_restatement(K, n):
    for th in (0, FULL, 1 << 17, 1 << 23):
        for begin in (0, 1000):
            for seed, draw in ((77, 5), ((1 << 40) + 3, (1 << 33) + 1)):
                want = SR.inject_list(n, begin, seed, draw, th)
                got = [K.inject_list(n, seed, draw, th, slot_begin=begin, max_blocks=mb).cpu().numpy() for mb in (0, 1, 3)]
                for g in got:          # the launcher's grid, one workgroup for every tile, three workgroups
                    assert g.dtype == np.int32 and np.array_equal(g, want), (n, th, begin, seed)
                if th == FULL:
                    assert np.array_equal(want, np.arange(n))
                if th == 0:
                    assert len(want) == 0
    # the list is the set of slots the plain injection writes
    maps = _road_maps(67, 131, 3, 1)
    st = _states(n, 10 + n)
    after, cnt = RR.inject(st, n, 1000, RR.road_cells(maps), 131, 1.0, 77, 5, 1 << 23, 1)
    changed = np.flatnonzero(after["init_x_px"] != st["init_x_px"])
    assert np.array_equal(SR.inject_list(n, 1000, 77, 5, 1 << 23), changed) and cnt == len(changed)


# ---- the candidates kernel -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_map(K):
    maps = _road_maps(67, 131, 3, 1)          # an odd number of columns
    return maps, {res: _dev_map(K, maps, res) for res in (1.0, 2.0)}, RR.road_cells(maps)


@pytest.mark.parametrize("C_", [1, 2, 3, 64, 65, 200])
def test_candidates_equal_the_restatement(K, odd_map, C_):
    maps, dms, road_h = odd_map
    n, cap = 300, 307
    st = _states(n, 3)
    planes = K.to_device(_to_planes(st, cap, SENT))
    for mode, begin, seed, draw, res in ((0, 0, 9, 4, 1.0), (1, 0, 9, 4, 2.0), (1, 1000, (1 << 50) + 1, (1 << 32) + 7, 2.0)):
        road = K.road_cells(dms[res])
        lst_h = SR.inject_list(n, begin, seed, draw, 1 << 22)
        lst = K.inject_list(n, seed, draw, 1 << 22, slot_begin=begin)
        assert np.array_equal(lst.cpu().numpy(), lst_h) and len(lst_h) > 66      # more entries than a wave
        first, m = 1, len(lst_h) - 2
        cand_cap = m * C_ + 5
        cst = K.to_device(np.full((7, cand_cap), SENT, F32))
        K.inject_candidates(planes, n, lst, first, m, C_, dms[res], road, seed, draw, mode, cst, slot_begin=begin)
        want = SR.candidates(st, lst_h[first:first + m], C_, begin, road_h, 131, res, seed, draw, mode)
        got = cst.cpu().numpy()
        assert got[:, :m * C_].tobytes() == _planes_of(want).tobytes(), (C_, mode, begin)
        assert (got[:, m * C_:] == SENT).all()
    assert planes.cpu().numpy().tobytes() == _to_planes(st, cap, SENT).tobytes()      # the slots are read, not written


# ---- the select kernel ---------------------------------------------------------------------------------------------------------------
def _weight_rows(m, C_, rng):
    w = rng.uniform(0.5, 9.0, (m, C_)).astype(F32)
    j = np.arange(C_)
    w[0, :] = 3.0                                        # every candidate ties: the first
    w[1, :] = NAN                                        # all NaN: candidate 0
    w[2, :] = 0.0                                        # all gated: the first
    w[3, :] = np.where(j % 2 == 0, NAN, 0.0)             # a 0 beats a NaN
    w[4, :] = 0.0
    w[4, C_ - 1] = 1e-30                                 # 0 loses to a positive weight, here the last candidate
    w[5, C_ // 2] = NAN                                  # a NaN in the middle
    top = w[6].max() + F32(1)
    w[6, [C_ - 1, C_ // 3]] = top                        # the maximum twice, in lanes apart (one a stride further for C > 64)
    w[7, :] = np.where(j == (C_ * 2) // 3, 7.0, NAN)     # the only number
    return w


@pytest.mark.parametrize("C_", [1, 4, 63, 64, 65, 200])
def test_select_picks_the_first_maximum(K, C_):
    import torch
    rng = np.random.default_rng(C_)
    n, cap, m, first = 40, 47, 11, 2                     # 11 waves: three workgroups, the last with three waves
    st = _states(n, 8)
    lst_h = np.sort(rng.choice(n, m + first + 1, replace=False)).astype(np.int32)
    w = _weight_rows(m, C_, rng)
    cand_cap = m * C_ + 3
    cand = rng.normal(0, 50, (7, cand_cap)).astype(F32)
    before = _to_planes(st, cap, SENT)
    planes, lst = K.to_device(before), K.to_device(lst_h)
    cst, cw = K.to_device(cand), K.to_device(np.concatenate([w.ravel(), np.full(3, 1e9, F32)]))
    pick, written = K.to_device(np.full(m + 1, -5, np.int32)), K.to_device(np.array([100], np.int64))
    K.inject_select(planes, n, lst, first, m, C_, cst, cw, pick=pick, written=written)
    want_pick = SR.pick(w)
    assert pick.cpu().numpy().tolist() == want_pick.tolist() + [-5], C_
    assert want_pick[:5].tolist() == [0, 0, 0, 1 if C_ > 1 else 0, C_ - 1] and want_pick[6] == min(C_ - 1, C_ // 3)
    want = before.copy()
    slots = lst_h[first:first + m]
    want[:, slots] = cand[:, np.arange(m) * C_ + want_pick]
    got = planes.cpu().numpy()
    assert got.tobytes() == want.tobytes(), C_                         # the written slots; the others and the padding as before
    assert int(written.item()) == 100 + m
    # no outputs asked for: the same slots
    planes2 = K.to_device(before)
    K.inject_select(planes2, n, lst, first, m, C_, cst, cw)
    assert planes2.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(cst.cpu(), torch.from_numpy(cand))


def test_launchers_refuse_bad_arguments(K, odd_map):
    import torch
    maps, dms, road_h = odd_map
    dm, L = dms[1.0], K.lib
    road = K.road_cells(dm)
    n, cap, m, C_ = 8, 8, 4, 3
    before = _to_planes(_states(n, 1), cap, 0.0)
    st = K.to_device(before)
    lst_b = np.array([0, 2, 3, 5, 6, -9, -9, -9], np.int32)
    cst_b, cw_b = np.full((7, 16), SENT, F32), np.full(16, 2.0, F32)
    lst, cst, cw = K.to_device(lst_b), K.to_device(cst_b), K.to_device(cw_b)
    cnt, ws = K.to_device(np.array([55], np.int64)), K.empty((64,), torch.uint8)
    pick = K.to_device(np.full(8, -5, np.int32))
    p = lambda t: vp(t.data_ptr()) if t is not None else None

    def do_list(n_=n, begin=0, th=FULL, out=lst, c=cnt, w=ws):
        return L.tdr_k_inject_list(n_, begin, 1, 2, th, p(out), p(c), p(w), 0, None)

    def do_cand(s=st, cap_=cap, n_=n, begin=0, l=lst, first=0, m_=m, c_=C_, desc=dm.desc, rd=road, n_road=None, mode=0, o=cst, ccap=16):
        return L.tdr_k_inject_candidates(p(s), cap_, n_, begin, p(l), first, m_, c_, C.byref(desc) if desc is not None else None, p(rd),
                                         road.numel() if n_road is None else n_road, 1, 2, mode, p(o), ccap, None)

    def do_sel(s=st, cap_=cap, n_=n, l=lst, first=0, m_=m, c_=C_, o=cst, ccap=16, w=cw):
        return L.tdr_k_inject_select(p(s), cap_, n_, p(l), first, m_, c_, p(o), ccap, p(w), p(pick), p(cnt), None)

    refused = [do_list(out=None), do_list(c=None), do_list(w=None), do_list(n_=-1), do_list(begin=-1), do_list(begin=(1 << 31) - 7),
               do_list(th=FULL + 1),
               do_cand(s=None), do_cand(l=None), do_cand(desc=None), do_cand(rd=None), do_cand(o=None), do_cand(n_=-1), do_cand(n_=9),
               do_cand(c_=0), do_cand(c_=4097), do_cand(mode=2), do_cand(mode=-1), do_cand(n_road=0), do_cand(n_road=67 * 131 + 1),
               do_cand(m_=6, ccap=17), do_cand(first=-1), do_cand(m_=-1), do_cand(first=6, m_=3), do_cand(begin=-1),
               do_sel(s=None), do_sel(l=None), do_sel(o=None), do_sel(w=None), do_sel(n_=-1), do_sel(n_=9), do_sel(c_=0), do_sel(c_=4097),
               do_sel(m_=6, ccap=17), do_sel(first=-1), do_sel(m_=-1), do_sel(first=6, m_=3)]
    assert refused == [-1] * len(refused), refused
    K.synchronize()
    assert st.cpu().numpy().tobytes() == before.tobytes() and lst.cpu().numpy().tobytes() == lst_b.tobytes()
    assert cst.cpu().numpy().tobytes() == cst_b.tobytes() and int(cnt.item()) == 55 and (pick.cpu().numpy() == -5).all()
    # empty calls are valid: the list's length alone; no candidate, no slot
    assert do_list(n_=0) == 0 and int(cnt.item()) == 0
    cnt.fill_(55)
    assert do_list(th=0) == 0 and int(cnt.item()) == 0
    cnt.fill_(55)
    assert do_cand(m_=0) == 0 and do_sel(m_=0) == 0
    K.synchronize()
    assert st.cpu().numpy().tobytes() == before.tobytes() and cst.cpu().numpy().tobytes() == cst_b.tobytes() and int(cnt.item()) == 55
    assert L.tdr_inject_list_workspace_bytes(4097) >= 8 * 17 and L.tdr_inject_list_workspace_bytes(-1) == 0


# ---- the handle against the device's own scorer --------------------------------------------------------------------------------------
N_S = 1024          # the candidates of a call (about 30 slots x 64) are more than the filter holds: several scoring rounds
P_S = 0.03


@pytest.fixture(scope="module")
def scene():
    from top_down_renderer_amd import synth
    return synth.make_scene(synth.Config("recovery", 4000, 4, 36, 12, 300, 4096, seed=41, res=2.0))


def _prepared(scene, kind, seed=5):
    """A filter after one update (draw = 1), and its renderer."""
    f, r = _handle(scene, kind, N_S, seed=seed)
    f.set_states(_spread_states(scene, N_S, 7, kind != "fixed"))
    f.propagate(0.3, 0.1, 0.005)
    f.update(r, scene.cfg.res)
    return f, r


def _device_scorer(scene, kind, r):
    """score(candidates) of the restatement through a SECOND filter of the same kind, map, parameters and particle count:
    set_states + compute_weights, N_S candidates a round (the last round padded with its first candidate)."""
    twin, _ = _handle(scene, kind, N_S, seed=99)

    def score(cand):
        ws, after = [], []
        for lo in range(0, len(cand), N_S):
            part = cand[lo:lo + N_S]
            full = np.concatenate([part, np.repeat(part[:1], N_S - len(part))])
            twin.set_states(full)
            twin.compute_weights(r, scene.cfg.res)
            ws.append(twin.raw_weights(N_S)[:len(part)])
            after.append(twin.states()[:len(part)])
        return np.concatenate(ws), np.concatenate(after)
    return score


def _expected(scene, cur, draw, mode, C_, seed, score, p=P_S):
    road = RR.road_cells(scene.class_maps)
    return SR.inject_sensor(cur, len(cur), 0, road, scene.cfg.map_size, scene.cfg.map_resolution, seed, draw, RR.threshold(p), mode,
                            C_, score)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["polar", "fixed", "cart"])
def test_handle_equals_the_restatement_over_the_devices_scorer(scene, kind, mode):
    (f, r), (g, _) = _prepared(scene, kind), _prepared(scene, kind)         # g: the same calls in chunks, on copies
    score = _device_scorer(scene, kind, r)
    chunk0 = f.L.tdr_config_tuning(b"inject_cand_chunk", -1)
    assert chunk0 == 65536 and g.step_count() == f.step_count() == 1        # the draw is the update count
    try:
        for C_, seed in ((1, 11), (5, (1 << 40) + 3), (64, 12)):
            before = _snapshot(f, states=False)
            cur = f.states()
            want, lst, picks = _expected(scene, cur, f.step_count(), mode, C_, seed, score)
            assert 20 <= len(lst) <= 40
            got_cnt = f.inject_sensor(r, scene.cfg.res, P_S, C_, mode, seed)
            got = f.states()
            assert got_cnt == len(lst) and got.tobytes() == want.tobytes(), (kind, mode, C_)
            assert _snapshot(f, states=False) == before, (kind, mode, C_)
            if C_ > 1:
                assert (picks > 0).sum() > len(lst) // 2                    # the tournaments do choose
            for chunk in (-(-len(lst) // 3) * C_, max(C_ - 1, 1)):          # three chunks; a chunk smaller than C (a slot each)
                assert f.L.tdr_config_tuning(b"inject_cand_chunk", chunk) == chunk
                g.set_states(cur)
                assert g.inject_sensor(r, scene.cfg.res, P_S, C_, mode, seed, count=False) is None
                assert g.states().tobytes() == want.tobytes(), (kind, mode, C_, chunk)
            f.L.tdr_config_tuning(b"inject_cand_chunk", chunk0)
    finally:
        f.L.tdr_config_tuning(b"inject_cand_chunk", chunk0)
    # the next update searches again where a gated winner stayed without a heading; its survivors all have one
    f.update(r, scene.cfg.res)
    assert (f.states()["have_init"] == 1).all() and f.step_count() == 2


@pytest.mark.parametrize("kind", ["polar", "fixed", "cart"])
def test_one_candidate_is_the_plain_injection(scene, kind):
    res = scene.cfg.res
    (a, r), (b, _) = _prepared(scene, kind), _prepared(scene, kind)
    assert a.states().tobytes() == b.states().tobytes()
    # mode 1: byte for byte tdr_filter_inject
    assert a.inject_sensor(r, res, 0.25, 1, 1, 31) == b.inject(0.25, 1, 31) > 100
    assert a.states().tobytes() == b.states().tobytes()
    # mode 0: the slot holds what the plain injection and the next scoring's search leave
    cnt = a.inject_sensor(r, res, 0.25, 1, 0, 32)
    assert cnt == b.inject(0.25, 0, 32) > 100
    b.compute_weights(r, res)
    sa, sb = a.states(), b.states()
    assert sa.tobytes() == sb.tobytes()
    a.compute_weights(r, res)
    assert a.states().tobytes() == sb.tobytes()
    # ... and the weights of the scoring after it.  One difference is the definition's: a search that finds no finite
    # candidate leaves theta = 0, have_init = 1 and, in the call that ran it, the reference's 1 / (FLT_MAX + regularization);
    # the same particle scored again, now with a heading, is "too much unknown", a NaN.  b's weights are those of the call
    # that searched, a's of a call after the search.
    wa, wb = a.raw_weights(N_S), b.raw_weights(N_S)
    diff = wa.view(np.uint32) != wb.view(np.uint32)
    no_finite = F32(1) / np.finfo(F32).max
    assert np.isnan(wa[diff]).all() and (wb[diff] == no_finite).all() and diff.sum() < cnt, (int(diff.sum()), wa[diff], wb[diff])
    b.compute_weights(r, res)
    assert b.raw_weights(N_S).tobytes() == wa.tobytes() and b.states().tobytes() == sb.tobytes()
    # p = 0: a valid call that writes nothing
    assert a.inject_sensor(r, res, 0.0, 8, 0, 1) == 0 and a.states().tobytes() == sb.tobytes()


def test_the_scan_as_images_and_the_kept_scan(scene):
    res = scene.cfg.res
    (a, r), (b, _), (c, _) = (_prepared(scene, "fixed") for _ in range(3))
    imgs = r.get_render()[0]
    want_cnt = a.inject_sensor(r, res, P_S, 8, 0, 5)
    assert b.inject_sensor(imgs, res, P_S, 8, 0, 5) == want_cnt and b.states().tobytes() == a.states().tobytes()
    with pytest.raises(Exception, match="no scan"):
        c.inject_sensor(None, res, P_S, 8, 0, 5)                # updated from a renderer: the filter kept no scan of its own
    c.compute_weights(imgs, res)
    assert c.inject_sensor(None, res, P_S, 8, 0, 5) == want_cnt and c.states().tobytes() == a.states().tobytes()


def test_recovery_step_sensor_tracks_injects_and_resets(scene):
    from top_down_renderer_amd._lib import RecoveryParamsC, RecoveryStateC
    res = scene.cfg.res
    (f, r), (g, _) = _prepared(scene, "fixed"), _prepared(scene, "fixed")
    rp = RecoveryParamsC(0.25, 0.5, 0.25, 0, 99)
    s, t = RecoveryStateC(0.0, 0.0), RR.Tracker(0.25, 0.5, 0.25)
    w = float(f.weight_stats()[2])
    before = f.states()
    assert f.recovery_step_sensor(s, rp, 8, r, res) == (0.0, 0) and t.track(w) == 0.0
    assert (s.w_slow, s.w_fast) == (w, w) and f.states().tobytes() == before.tobytes()
    s.w_slow, s.w_fast = 4 * w, 2 * w
    t.w_slow, t.w_fast = 4 * w, 2 * w
    p = t.track(w)
    assert 0 < p <= 0.25
    cnt = g.inject_sensor(r, res, p, 8, 0, 99)
    assert f.recovery_step_sensor(s, rp, 8, r, res) == (p, cnt) and cnt > 0
    assert f.states().tobytes() == g.states().tobytes() and (s.w_slow, s.w_fast) == (0.0, 0.0)


def test_handle_refusals_write_nothing(scene):
    from top_down_renderer_amd import batch
    from top_down_renderer_amd._lib import RecoveryParamsC, RecoveryStateC
    from top_down_renderer_amd.particle_filter import FilterParams
    res = C.c_float(scene.cfg.res)
    f, r = _prepared(scene, "polar")
    L = f.L
    before = _snapshot(f)
    out, pout = C.c_int64(777), C.c_double(777.0)
    state, ok = RecoveryStateC(3.0, 1.0), RecoveryParamsC(0.001, 0.1, 0.5, 0, 1)
    nan, inf = float("nan"), float("inf")

    def refused(rc, word):
        assert rc == -1 and word in L.tdr_last_error().decode(), L.tdr_last_error()
        assert out.value == 777 and pout.value == 777.0 and (state.w_slow, state.w_fast) == (3.0, 1.0)
        assert _snapshot(f) == before

    def inj(h=f.h, rh=r.h, rs=res, p=0.5, c=8, mode=0):
        return L.tdr_filter_inject_sensor(h, None, rh, rs, C.c_double(p), c, mode, 1, C.byref(out))

    def step(h=f.h, st=state, rp=ok, c=8, rh=r.h, rs=res):
        return L.tdr_filter_recovery_step_sensor(h, C.byref(st) if st is not None else None, C.byref(rp) if rp is not None else None, c,
                                                 None, rh, rs, C.byref(pout), C.byref(out))

    refused(inj(h=None), "null")
    for p in (-0.001, 1.001, nan, inf):
        refused(inj(p=p), "p =")
    for mode in (-1, 2):
        refused(inj(mode=mode), "heading_mode")
    for c in (0, -1, 4097):
        refused(inj(c=c), "candidates")
        refused(step(c=c), "candidates")
    for bad in (0.0, -1.0, nan, inf):
        refused(inj(rs=C.c_float(bad)), "res =")
        refused(step(rs=C.c_float(bad)), "res =")
    refused(inj(rh=None), "no scan")                             # the filter kept no scan: it was updated from the renderer
    refused(step(h=None), "null")
    refused(step(st=None), "null")
    refused(step(rp=None), "null")
    refused(step(rp=RecoveryParamsC(0.0, 0.1, 0.5, 0, 1)), "alpha_slow")
    refused(step(rp=RecoveryParamsC(0.001, 0.1, 0.5, 2, 1)), "heading_mode")
    other = batch.Renderer(scene.lut)                             # a render of another shape; a renderer without a render
    refused(inj(rh=other.h), "no scan")
    other.render_polar(scene.pts, 4, 3, scene.cfg.res, float(scene.cfg.ang_res), scene.cfg.ncls, scene.cfg.nb, scene.cfg.nr + 1)
    refused(inj(rh=other.h), "shape")
    e, _ = _handle(scene, "polar", 64)
    refused(inj(h=e.h), "no particles")
    g, _ = _handle(scene, "polar", 64, seed=6)
    g.set_states(_spread_states(scene, 64, 3, True))
    refused(step(h=g.h), "no update")
    noroad = batch.MapHandle(np.full((scene.cfg.ncls, 50, 50), 9.0, F32), np.zeros((50, 50), np.uint8))
    noroad.sample_pts_polar(scene.cfg.nb, scene.cfg.nr, float(scene.cfg.ang_res))
    h = batch.FilterHandle(noroad, 64, FilterParams(fixed_scale=1.0), seed=1)
    h.set_states(_spread_states(scene, 64, 3, False))
    hb = h.states().tobytes()
    refused(inj(h=h.h), "no road")
    assert h.states().tobytes() == hb
    # outputs are optional
    assert L.tdr_filter_inject_sensor(f.h, None, r.h, res, C.c_double(0.0), 8, 0, 1, None) == 0 and _snapshot(f) == before


def test_a_sharded_filter_is_refused(scene):
    """One rank over the callback transport, as tests/test_recovery.py builds it."""
    from top_down_renderer_amd import FilterParams
    from top_down_renderer_amd._lib import RecoveryParamsC, RecoveryStateC, check
    f, r = _handle(scene, "polar", 64)
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
        st = np.ascontiguousarray(_spread_states(scene, 64, 2, False))
        check(L.tdr_filter_set_states(sh, st.ctypes.data_as(vp), 64))
        out = C.c_int64(777)
        assert L.tdr_filter_inject_sensor(sh, None, r.h, C.c_float(scene.cfg.res), C.c_double(0.5), 8, 0, 1, C.byref(out)) == -1
        assert "sharded" in L.tdr_last_error().decode() and out.value == 777
        state, ok = RecoveryStateC(0.0, 0.0), RecoveryParamsC(0.001, 0.1, 0.5, 0, 1)
        assert L.tdr_filter_recovery_step_sensor(sh, C.byref(state), C.byref(ok), 8, None, r.h, C.c_float(scene.cfg.res), None, None) == -1
        assert "sharded" in L.tdr_last_error().decode()
        got = np.zeros(64, RR.STATE_DTYPE)
        check(L.tdr_filter_get_states(sh, got.ctypes.data_as(vp), 64))
        assert got.tobytes() == st.tobytes()
    finally:
        L.tdr_filter_destroy(sh)
        L.tdr_comm_destroy(comm)


# ---- the kidnapped robot's scan: the CPU oracle's picks, and what the feature is for ---------------------------------------------------
KID_P, KID_C, KID_SEED = 0.05, 64, 1
BASIN_PX = 12.0


@pytest.fixture(scope="module")
def kidnapped():
    """The c1 scene, 4000 particles condensed on its first pose, and the scan of tests/test_recovery.py::kidnap_run's second
    pose; one handle call with C = 64 and one with C = 1 on copies."""
    from top_down_renderer_amd import batch, synth
    from top_down_renderer_amd.particle_filter import FilterParams
    sc = synth.make_scene("c1", n_particles=4000)
    cfg = sc.cfg
    rng = np.random.default_rng(77)
    while True:
        pose2 = synth.pick_true_pose(sc.lab, rng, 168)
        if np.hypot(pose2[0] - sc.pose[0], pose2[1] - sc.pose[1]) >= 400:
            break
    pts2 = synth.make_scan(cfg, sc.lab, pose2, rng)
    st = synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(78), n=4000, uniform_frac=0.0)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, cfg.map_resolution)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    r = batch.Renderer(sc.lut)
    r.render_polar(pts2, 4, 3, cfg.res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    out = {}
    for C_ in (KID_C, 1):
        f = batch.FilterHandle(m, 4000, FilterParams(fixed_scale=1.0), seed=5)
        f.set_states(st)
        cnt = f.inject_sensor(r, cfg.res, KID_P, C_, 0, KID_SEED)
        out[C_] = (cnt, f.states())
    return sc, pose2, pts2, st, out


def _near(states, pose, radius):
    x = states["dx_m"] * states["scale"] + states["init_x_px"]
    y = states["dy_m"] * states["scale"] + states["init_y_px"]
    return np.hypot(x - pose[0], y - pose[1]) < radius


def test_picks_are_the_cpu_oracles(kidnapped, oracle):
    """The oracle scores the restatement's candidates (its own 40-rotation search).  Where its best and second-best weight
    of a slot are further apart than 1e-4 relative — ten times the 1e-5 weight tolerance of the parity tests — the slot
    holds the oracle's pick; at most 1 % of the slots may fall under that gap."""
    sc, pose2, pts2, st, out = kidnapped
    cfg = sc.cfg
    road = RR.road_cells(sc.class_maps)
    lst = SR.inject_list(4000, 0, KID_SEED, 0, RR.threshold(KID_P))
    cand = SR.candidates(st, lst, KID_C, 0, road, cfg.map_size, cfg.map_resolution, KID_SEED, 0, 0)
    om = oracle.OracleMap(sc.class_maps, sc.class_mask, cfg.map_resolution)
    fp = oracle.make_params(cfg.ncls, fixed_scale=1.0)
    scan = oracle.raster_polar(pts2, cfg.res, cfg.ang_res, sc.lut, cfg.ncls, cfg.nb, cfg.nr)
    tab = oracle.polar_table(cfg.nb, cfg.nr, cfg.ang_res, cfg.map_resolution)
    flat = np.ascontiguousarray(cand.reshape(-1).astype(oracle.STATE_DTYPE))
    w = np.asarray(oracle.compute_weights(om, tab, cfg.nb, cfg.nr, scan, cfg.res, fp, flat), F32).reshape(len(lst), KID_C)
    picks = SR.pick(w)
    key = np.sort(np.where(np.isnan(w), F32(-1), w).astype(np.float64), axis=1)
    clear = (key[:, -1] - key[:, -2]) > 1e-4 * np.abs(key[:, -1])
    cnt, got = out[KID_C]
    assert cnt == len(lst) and 150 < cnt < 250
    win = cand[np.arange(len(lst)), picks]
    same = (got["init_x_px"][lst] == win["init_x_px"]) & (got["init_y_px"][lst] == win["init_y_px"])
    cpu_near = int(_near(win, pose2, BASIN_PX).sum())
    print(f"slots {cnt}, under the gap {int((~clear).sum())}, oracle picks kept {int(same.sum())}, oracle winners within "
          f"{BASIN_PX} px of the new pose {cpu_near}, device {int(_near(got, pose2, BASIN_PX).sum())}")
    assert (~clear).sum() <= len(lst) // 100
    assert same[clear].all(), np.flatnonzero(clear & ~same)
    rest = np.setdiff1d(np.arange(4000), lst)
    assert got[rest].tobytes() == st[rest].tobytes()


def test_one_call_finds_the_basin_the_uniform_draw_misses(kidnapped):
    """p = 0.05, mode 0 on the kidnapped scan.  The seed was fixed with the CPU restatement over the oracle's weights: seed 1
    gives 209 slots, 20 winners within 12 px of the new pose (33 within 40 px) against 0 for the slots' first candidates,
    which are the uniform injection, and a smallest best-to-second gap of 4.0e-4 (seeds 2 and 2026: 8 and 17 winners, gaps
    2.0e-4 and 1.1e-4).  Measured on the MI355X: 20 against 0.  The device's picks are pinned by the equality tests and by
    test_picks_are_the_cpu_oracles, which prints both counts; the bound here is only that the call shows the basin."""
    sc, pose2, pts2, st, out = kidnapped
    assert not _near(st, pose2, 200.0).any()                   # the cloud is condensed elsewhere
    many, one = out[KID_C], out[1]
    assert many[0] == one[0]                                   # the same slots
    n_many, n_one = int(_near(many[1], pose2, BASIN_PX).sum()), int(_near(one[1], pose2, BASIN_PX).sum())
    print(f"within {BASIN_PX} px of the new pose: C = {KID_C}: {n_many}, C = 1: {n_one} (of {many[0]} slots)")
    assert n_many >= 3 and n_one == 0
