"""A long-lived BATCH of filter handles driven through a script of events with the CPU oracle in lock step (shared by
tests/test_batch_session.py; not a test module).

A `Fleet` owns what a node of many robots owns for hours: one batch.MapHandle, K `session_ref.Session` objects that share
it (each with its own FilterHandle, Renderer, parameters, seed and oracle mirror) and a caller's stream.  The members are
driven with the batched calls of top_down_renderer_amd/batch.py — step_batch, render_batch, pose_batch, compute_gmm_batch —
and every member is then checked by the stage checks of its own Session, each stage on inputs READ BACK from the device:

  propagate    the oracle propagates the states read back BEFORE the call on the member's mirrored oracle.Rng;
               last_dist bit for bit, last_dist behind n untouched.  (The propagated states cannot be read after a batched
               step: they are held to the oracle through the score and the gather below.)
  score        a fresh twin (new MapHandle, new FilterHandle) with set_states(the oracle's propagated states) runs
               compute_weights: the batched filter's raw weights are the twin's bits; Session._check_score holds them to
               the oracle within WEIGHT_RTOL with the NaN and zero pattern, the search by TIE_RTOL
  statistics / resample / gather / pose: Session.check_update and Session.pose, unchanged

batch.last_stats() must be the (batched, standalone) pair the script's row states; the row's reasons are checked against
a model of batch_eligible() kept HERE from the mirrors (the generator mode, the count, the un-initialised flag and the two
process-wide switches) — never against the library.  A member the row expects to take its standalone calls inside the
batched call gets the same checks; one on the device's own noise (configure(0)) cannot have its propagated states
predicted, so its call is held to what stays knowable: last_dist finite, the statistics on the raw weights read back, the
resample on the mirrored uniform (the host generator serves it in that mode), the fields the noise does not touch
gathered by the oracle's indices, the counts, the pose.

With handle=False the same script runs on the oracle alone (no GPU) and `records` / `calls` hold what
tests/test_batch_session.py asserts about the script itself."""
import numpy as np

import session_ref as S

F32 = np.float32
MOTION = (0.3, 0.1, 0.01)


def _res(k):
    return 0.8 + 0.05 * (k % 9)


class Fleet:
    """members: [dict(name, n_max, seed, params, cart=False)] — the first polar member's Session makes the map."""

    def __init__(self, oracle, spec, members, handle, shape=(36, 12), name="fleet", cart_spec=None):
        self.oracle, self.handle, self.name, self.shape = oracle, handle, name, tuple(shape)
        self.ses, self.order = {}, []
        self.map_handle = None
        for m in members:
            cart = bool(m.get("cart"))
            s = S.Session(oracle, cart_spec if cart else spec, m["n_max"], m["seed"], m["params"], cart=cart, handle=handle,
                          shape=(48, 64) if cart else self.shape, map_handle=self.map_handle, name=f"{name}.{m['name']}")
            if self.map_handle is None:
                self.map_handle = s.map_handle
            self.ses[m["name"]] = s
            self.order.append(m["name"])
        self.uninit = {k: True for k in self.ses}       # the mirror of tdr_filter::maybe_uninit (a fresh handle: true)
        self.rendered = {}                               # member -> (flat, res) of its renderer's batched render
        self.adaptive = {}                               # member -> adaptive_count() after the last batched fit
        self.calls = []                                  # one record per batched step call
        self.k = 0                                       # steps made: the next `res`
        self._stream = None
        if handle:
            from top_down_renderer_amd import _lib, batch
            self.batch, self.TdrError = batch, _lib.TdrError

    # ---- helpers ------------------------------------------------------------------------------------------------------
    def stream(self, own):
        if not own or not self.handle:
            return None
        if self._stream is None:
            import torch
            self._stream = torch.cuda.Stream()
        return self._stream.cuda_stream

    def gated(self, name):
        p = self.ses[name].params
        return bool(p.get("force_on_map")) or p.get("fixed_scale", 1.0) < 0

    def scored(self, name):
        """What a scoring call leaves of maybe_uninit: the search initialises every un-gated particle."""
        if not self.gated(name):
            self.uninit[name] = False

    def eligible(self, name, sw):
        """batch_eligible() from the mirrors.  The float / integer form (tdr_su_shape_ok, score_ws): shift_uniform 0: never
        the integer form; 2: always (these maps have a compact form, four-ring groups, nb <= 4095); 1, the default: only
        with nb * nr >= 8192 bins AND n >= 64 * nb — so at 36 x 12 the count never flips the form, at 128 x 64 it does at
        8192 = 64 x 128."""
        s = self.ses[name]
        n = len(s.st)
        nb, nr = s.shape
        mode = sw["shift_uniform"]
        integer = mode == 2 or (mode == 1 and nb * nr >= 8192 and n >= 64 * nb)
        return (s.parity and (not self.uninit[name] or sw["batch_init_search"] == 1) and 1 <= n <= 32768 and not integer)

    # ---- the batched step --------------------------------------------------------------------------------------------
    def step(self, members, n_targets, sources, stream, expect, sw, zero=(), degenerate=(), search=(), why=None, tag=""):
        """One batch.step_batch for `members` in this order.  expect: the (batched, standalone) pair the row states; why:
        {member: reason} for the members the row expects to go standalone (and, in script F, the reason a batched member
        exercises)."""
        o, why = self.oracle, dict(why or {})
        jobs, scans, resv, nts = [], [], [], []
        modes = {}
        for j, (name, nt, src) in enumerate(zip(members, n_targets, sources)):
            s = self.ses[name]
            s.label = tag
            n = len(s.st)
            assert not s.cart, (tag, name)
            modes[name] = "B" if self.eligible(name, sw) else "S"
            if n == 0:                                     # a handle without particles: its standalone calls, which do nothing
                res = _res(self.k + j)
                if self.handle:
                    scans.append(S.images(s.scan_flat(res), *s.shape))
                jobs.append((name, s, 0, nt, src, None, res, None, None))
                resv.append(res)
                nts.append(nt)
                continue
            if isinstance(nt, tuple):                      # ("adaptive", stand-in for the oracle-alone run)
                nt = self.adaptive[name] if self.handle else nt[1]
                assert 1 <= nt <= s.n_max, (tag, name, nt)
            if self.handle:
                got = s.f.states()
                assert got.tobytes() == s.st.tobytes(), (s._what("before the batched step"), S.bits_equal(got, s.st))
            if src == "batched":
                flat, res = self.rendered[name]
            else:
                res = _res(self.k + j)
                flat = s.scan_flat(res, name in zero)
            ref = s.st.copy()
            last = o.propagate(ref, *MOTION, s.frozen, s.fpo, s.rng if s.parity else s.side)
            if self.handle:
                scans.append(s.renderer if src == "batched" else s._scan_arg(flat, res, "renderer" if src == "renderer" else "host"))
            jobs.append((name, s, n, nt, src, flat, res, ref, last))
            resv.append(res)
            nts.append(nt)
        n_b = sum(m == "B" for m in modes.values())
        assert (n_b, len(members) - n_b) == tuple(expect), (tag, "the row's expectation is not the eligibility rule's", modes, expect)
        assert {k for k, m in modes.items() if m == "S"} == {k for k, v in why.items() if v[0] == "S"}, (tag, modes, why)
        if self.handle:
            got = self.batch.step_batch([self.ses[m].f for m in members], scans, resv, [MOTION] * len(members), nts,
                                        stream=self.stream(stream))
            assert got == tuple(expect), (tag, "last_stats", got, expect)
            assert self.batch.last_stats() == tuple(expect), tag
        self.k += 1
        self.calls.append(dict(tag=tag, members=list(members), k=len(members), expect=tuple(expect), modes=modes, why=why,
                               stream=bool(stream), sources=list(sources)))
        for name, s, n, nt, src, flat, res, ref, last in jobs:
            if n == 0:
                s.unchanged("a batched step of a handle without particles")
                continue
            if self.handle:
                what = s._what("propagate (batched step)")
                ld = s.f.last_dist(n)
                if s.parity:
                    assert ld.tobytes() == last.tobytes(), (what, "last_dist", int((ld != last).sum()))
                else:
                    assert np.isfinite(ld).all(), what
                tail = s.f.last_dist(s.n_max)[n:]
                assert tail.tobytes() == s.ld[n:].tobytes(), (what, "last_dist behind n was written")
                if src == "batched":
                    img, _ = s.renderer.get_render()
                    assert np.array_equal(img, S.images(flat, *s.shape)), s._what("batched render")
            else:
                ld = last
            s.ld[:n] = ld
            deg = name in degenerate
            if self.handle and not s.parity:
                self._check_device_noise(s, n, nt, ld, res, src, deg)
            else:
                s.check_update(ref, ld.copy(), flat, res, nt, source=src, degenerate=deg, stage="batched update")
            self.scored(name)
            s.records[-1].update(call=len(self.calls) - 1, want_search=name in search, mode=modes[name], why=why.get(name),
                                 zero=name in zero)

    def _check_device_noise(self, s, n, n_target, ld, res, src, degenerate):
        """A member on the device's own noise (its standalone calls inside the batched call): see the module's docstring."""
        o, f, what = self.oracle, s.f, s._what("batched update on the device's own noise")
        before = s.st
        n_new = n if n_target < 0 else max(1, min(int(n_target), s.n_max))
        raw = f.raw_weights(n)
        w = f._floats(f.L.tdr_filter_get_weights, n)
        idx, after = f.resample_indices(), f.states()
        assert f.num_particles() == n_new == len(after) and f.step_count() == s.steps + 1, what
        with np.errstate(all="ignore"):
            w_o, _, _ = o.update_weights(raw, ld)
        assert np.allclose(w, w_o, rtol=S.STATS_RTOL, atol=0), (what, "weights")
        idx_o = o.resample_prefix(w, n_new, s.rng.uniform())
        assert np.array_equal(idx, idx_o), (what, "resample indices", int((idx != idx_o).sum()))
        keep = ("init_x_px", "init_y_px", "have_init") + (("scale",) if s.frozen else ())
        bad = S.bits_equal(after, o.gather_states(before, idx_o), keep)
        assert not bad, (what, "gather of the fields the noise does not touch", bad)
        assert all(np.isfinite(after[k]).all() for k in S.FIELDS), what
        ms, _ = f.mean_cov(True)
        assert np.isfinite(ms).all(), what
        s.ml, s.st = ms, after
        s.steps += 1
        good = float((np.isfinite(raw) & (raw != 0)).mean())
        s.records.append(dict(label=s.label, n=n, n_new=n_new, good=good, distinct=len(np.unique(idx)), search=0.0,
                              degenerate=degenerate, source=src, geo=False, res=res, shape=s.shape, ncls=s.spec.ncls,
                              parity=False))
        s.pose("pose after update")

    # ---- the other batched calls ---------------------------------------------------------------------------------------
    def render(self, members, stream=False, empty=None, verify=True, tag=""):
        """One batch.render_batch: clouds of different lengths (member j drops the last 41 j points), `empty` gets none.
        verify=False leaves the renders unread — the next step reads them with no host synchronisation in between and
        checks the images afterwards."""
        o = self.oracle
        clouds, resv = [], []
        s0 = self.ses[members[0]]
        for j, name in enumerate(members):
            s = self.ses[name]
            pts = np.ascontiguousarray(s.spec.pts[: len(s.spec.pts) - 41 * j], F32)
            res = _res(self.k + 2 * j + 1)
            flat = o.raster_polar(pts, res, s.ang_res, s._lut(), s.spec.ncls, *s.shape)
            if name == empty:
                pts, flat = pts[:0], np.zeros_like(flat)
            clouds.append((pts, pts.shape[1], 3))
            resv.append(res)
            self.rendered[name] = (flat, res)
        assert len({len(c[0]) for c in clouds}) == len(clouds), (tag, "clouds of different lengths")
        if self.handle:
            self.batch.render_batch([self.ses[m].renderer for m in members], clouds, resv, s0.ang_res, s0.spec.ncls, *s0.shape,
                                    stream=self.stream(stream))
            if verify:
                for name in members:
                    s = self.ses[name]
                    img, _ = s.renderer.get_render()
                    assert np.array_equal(img, S.images(self.rendered[name][0], *s.shape)), (tag, name, "batched render")

    def pose(self, members, stream=False, tag=""):
        """One batch.pose_batch: each record against the cache it fills (tdr_filter_mean_cov(f, 0) read afterwards), and —
        through Session.pose — against a fresh twin on the same states, pose_ref's bounds and tdr_filter_scale's rule."""
        if not self.handle:
            return
        ss = [self.ses[m] for m in members]
        for s in ss:
            s.label = tag
        mean, cov, scale, n = self.batch.pose_batch([s.f for s in ss], stream=self.stream(stream))
        for i, s in enumerate(ss):
            what = s._what("batched pose")
            assert n[i] == len(s.st), what
            fixed = s.params.get("fixed_scale", 1.0)
            want = F32(fixed) if fixed > 0 else (s.st["scale"][0] if s.frozen and len(s.st) else F32(-1))
            assert F32(scale[i]) == want and F32(s.f.scale()) == want, (what, "scale", scale[i], s.f.scale(), want)
            m0, c0 = s.f.mean_cov(False)       # the cache the call filled
            assert mean[i].tobytes() == m0.tobytes() and cov[i].tobytes() == c0.tobytes(), (what, "record against the cache")
            s.pose("pose after the batched pose")      # ... the twin's bits, pose_ref's bounds

    def gmm(self, members, stream=False, tag=""):
        """One batch.compute_gmm_batch: the mixture and the adaptive count are a fresh twin's compute_gmm(device=True) on
        the states read back (same n_max, same starting count).  The fit seeds from the samples (nearest to the mean, then
        farthest first: csrc/tdr_gmm.cpp) and draws nothing from the filter's generator: the mirror does not draw."""
        if not self.handle:
            return
        ss = [self.ses[m] for m in members]
        k0 = [s.f.num_gaussians() for s in ss]
        self.batch.compute_gmm_batch([s.f for s in ss], stream=self.stream(stream))
        for s, name, k in zip(ss, members, k0):
            s.label = tag
            what = s._what("batched gmm")
            tw = self.batch.FilterHandle(s.map_handle, s.n_max, s._fp_c(), seed=1)
            tw.set_states(s.st)
            tw.set_num_gaussians(k)
            tw.compute_gmm(device=True)
            (m, c), (mt, ct) = s.f.get_gmm(), tw.get_gmm()
            assert len(m) >= 1 and m.tobytes() == mt.tobytes() and c.tobytes() == ct.tobytes(), (what, "mixture", len(m), len(mt))
            assert s.f.num_gaussians() == tw.num_gaussians(), what
            self.adaptive[name] = s.f.adaptive_count()
            assert self.adaptive[name] == tw.adaptive_count(), (what, "adaptive count")
            s.unchanged("batched gmm")

    def refuse(self, kind, tag=""):
        """A call tdr_batch_step refuses; afterwards every member's states, weights and step count stand (the generators:
        the next step is bit for bit)."""
        if not self.handle:
            return
        polar = [m for m in self.order if not self.ses[m].cart and len(self.ses[m].st)]
        a, b = self.ses[polar[0]], self.ses[polar[1]]
        weights = {m: self.ses[m].f.weights() for m in polar}
        img = S.images(a.scan_flat(1.0), *a.shape)
        if kind == "twice":
            fs, scans = [a.f, b.f, a.f], [img, img, img]
        elif kind == "shape":
            r = self.batch.Renderer(a._lut())
            r.render_polar(a.spec.pts, 4, 3, 1.0, F32(2 * np.pi / 25), a.spec.ncls, 25, 16)
            fs, scans = [a.f, b.f], [img, r]
        else:
            c = [self.ses[m] for m in self.order if self.ses[m].cart][0]
            a._scan_arg(a.scan_flat(1.0), 1.0, "renderer")
            fs, scans = [a.f, c.f, b.f], [img, a.renderer, img]
        try:
            self.batch.step_batch(fs, scans, 1.0, [MOTION] * len(fs), stream=self.stream(kind == "shape"))
        except self.TdrError:
            pass
        else:
            raise AssertionError((tag, "tdr_batch_step accepted the call"))
        assert self.batch.last_stats() == (0, 0), tag
        for m, s in self.ses.items():
            s.label = tag
            s.unchanged("a refused batched step")
            if m in weights:
                assert np.array_equal(s.f.weights(), weights[m], equal_nan=True), (tag, m, "weights")

    # ---- events on the shared map ----------------------------------------------------------------------------------------
    def window(self, shape, tag=""):
        first = True
        for s in self.ses.values():
            if s.cart:
                continue
            if first:
                s.window(shape, tag)
                first = False
            else:
                s.label = tag
                s._set_shape(shape)
                s.unchanged("window")
        self.shape = tuple(shape)
        self.rendered.clear()

    def new_map(self, spec, how, via, patch=None, tag=""):
        """The map replaced ONCE through member `via` (whose particles the call shifts by the centre's move); the others'
        mirrors take the new map and the driver gives them their own states shifted alike through set_states."""
        old = self.ses[via].spec
        dx, dy = spec.center[0] - old.center[0], spec.center[1] - old.center[1]
        changed = self.ses[via].new_map(spec, how, tag, patch=patch)
        if self.handle and how == "patch":
            assert changed > 0, (tag, changed)
        if self.handle and how == "incremental":
            assert changed != 0, (tag, changed)
        for name, s in self.ses.items():
            if name == via or s.cart:
                continue
            s.unchanged("the map replaced through another member")
            s._set_oracle_map(spec)
            st = s.st.copy()
            self.oracle.shift_init(st, dx, dy)
            s.set_states(st, tag)
            self.uninit[name] = bool((st["have_init"] == 0).any())
        self.rendered.clear()
