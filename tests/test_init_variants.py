"""Every instantiation of the 40-rotation heading search (csrc/tdr_score_init.hip), proven to run and held to the exact
costs.  Run with `pytest -m gpu`.

tdr_score_init_pass picks one of four passes on the host — vector, matrix cores on pre-split half records, matrix cores
splitting the records on the fly, matrix cores on wide records — each a template, each with a batched twin; a matrix-core
pass whose scan counts do not fit f16 sends the search back through the vector kernel.  Per row of init_scenes.ROWS:
  * a COUNTED run (tdr_profile_enable(2)): slots [12..15] of tdr_profile_variants say which pass wrote the results of how
    many 64-particle batches — the row's pass, every batch with work, no other; the vector kernel's slot is 0 unless the
    row is a fallback row, where it too counts every batch;
  * an uncounted run: the same bits (theta, have_init, raw weights);
  * init_exact_ref.check_choice: gated particles untouched, particles no candidate can win at theta 0 with the weight
    1 / (FLT_MAX + regularization), every other theta bit-equal to a candidate that is the FIRST of its shift class and whose
    exact cost is within TAU = 2e-5 of the exact minimum (tests/test_init_exact_ref.py: in every scene that pins at least
    90 % of the headings to one value);
  * the raw weights within 1e-5 of the oracle's at the chosen theta.
The excess over the exact minimum and the duration of every row are printed (DESIGN.md 3.7 records them)."""
import ctypes as C
import time

import numpy as np
import pytest

import init_exact_ref as X
import init_scenes as S
from test_shift_uniform import tdr  # noqa: F401
from variant_scenes import counted

pytestmark = pytest.mark.gpu
_MAPS = {}


def _map(pkg, k, scene):
    if scene not in _MAPS:
        cfg, sc = S.scene(scene)
        m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), sc.class_maps, sc.class_mask, kernels=k)
        m.samplePtsPolar((cfg.nb, cfg.nr), cfg.ang_res)
        _MAPS[scene] = m
    return _MAPS[scene]


class _Switches:
    """init_mfma, rec16_min, init_ahead for the length of a row; put back whatever happens."""

    def __init__(self, k, mfma, rec16_min, ahead):
        self.lib, self.want = k.lib, (mfma, rec16_min, ahead)

    def __enter__(self):
        lib = self.lib
        self.old = (lib.tdr_config_init_mfma(-1), int(lib.tdr_config_rec16_min_particles(-1)),
                    int(lib.tdr_config_tuning(b"init_ahead", -1)))
        lib.tdr_config_init_mfma(self.want[0])
        lib.tdr_config_rec16_min_particles(self.want[1])
        assert lib.tdr_config_tuning(b"init_ahead", self.want[2]) == self.want[2]

    def __exit__(self, *exc):
        self.lib.tdr_config_init_mfma(self.old[0])
        self.lib.tdr_config_rec16_min_particles(self.old[1])
        self.lib.tdr_config_tuning(b"init_ahead", self.old[2])
        self.lib.tdr_profile_enable(0)


def _assert_weights(w, ref, rtol=1e-5):
    assert np.array_equal(np.isnan(w), np.isnan(ref)), (int(np.isnan(w).sum()), int(np.isnan(ref).sum()))
    ok = ~np.isnan(ref)
    err = np.abs(w[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    assert err.max(initial=0.0) <= rtol, f"max rel err {err.max():.3e}"


def _search(pkg, k, m, ref, us):
    """One standalone search + scoring launch: (theta, have_init, raw weights) on the host."""
    st, n = ref["st"], len(ref["st"])
    f = pkg.ParticleFilter(n, m, pkg.FilterParams(**ref["params"]), kernels=k, init_particles=False)
    f.set_states(st)
    k.score(m.dev, m.scan_handle(ref["scan"]), ref["cfg"].res, f.fp_c, f.st, n, f.raw_w, init_search=True,
            uniform_scale=1.0 if us else 0.0)
    got = k.states_to_host(f.st, n, st.dtype)
    return got["theta"].copy(), got["have_init"].copy(), f.raw_w[:n].cpu().numpy()


def _check_against_exact(oracle, ref, theta, have_init, raw):
    """check_choice, then the weights at the chosen theta against the oracle's; returns the largest excess."""
    se, st = ref["search"], ref["st"]
    worst = X.check_choice(se, st["theta"], theta, have_init, raw, ref["raw_o"], st["have_init"])
    st2 = st.copy()
    idx = se.searched()
    st2["theta"][idx], st2["have_init"][idx] = theta[idx], 1
    cfg = ref["cfg"]
    raw2 = oracle.compute_weights(ref["om"], ref["tab"], cfg.nb, cfg.nr, ref["scan"], cfg.res, ref["fpo"], st2)
    _assert_weights(raw, raw2)
    return worst


@pytest.mark.parametrize("row", S.ROWS, ids=lambda r: r["name"])
def test_variant_runs_and_chooses_exactly(tdr, oracle, row):
    pkg, k = tdr
    ref = S.reference(oracle, row["scene"], row["mode"], row["var"], row["kind"], row["k"])
    m = _map(pkg, k, row["scene"])
    if row["us"]:
        assert row["mode"] == "fixed" and (ref["st"]["scale"] == 1).all()
    t0 = time.perf_counter()
    with _Switches(k, row["mfma"], row["rec16_min"], row["ahead"]):
        on, v = counted(k, lambda: _search(pkg, k, m, ref, row["us"]))
        off = _search(pkg, k, m, ref, row["us"])
    gpu_s = time.perf_counter() - t0
    print(f"{row['name']}: pass counters [12..15] = {v[12:]}, both searches {gpu_s * 1e3:.0f} ms")
    batches = ref["search"].wanted_batches()
    want = [0, 0, 0, 0]
    want[row["slot"] - 12] = batches
    if row["fallback"]:
        want[S.VECTOR - 12] = batches
    assert v[12:] == want, f"pass counters {v[12:]}, expected {want} ({batches} batches with work)"
    for a, b, what in zip(on, off, ("theta", "have_init", "raw weights")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"counting changed {what}"
    worst = _check_against_exact(oracle, ref, *on)
    print(f"{row['name']}: largest excess over the exact minimum {worst:.3e} (allowed {X.TAU})")
    if row["slot"] == S.HALF:
        assert m.dev.rec16 is not None


# ---- the half records themselves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k2", [-10, 0, 10], ids=lambda e: f"weights_x_2^{e}")
@pytest.mark.parametrize("kind", ["w", "unit"])
@pytest.mark.parametrize("scene", ["c3", "c6", "c7"])
def test_half_records_are_hi_plus_lo(tdr, oracle, scene, kind, k2):
    """half_records_kernel: per cell  H_c + L_c = 2^e * float32(0.01 w_c) * d_c  to 2^-20 relative where d_c > 0 — e the
    one power of two that brings the largest 0.01 w_c into [1, 2) — or d_c itself to 2^-20 when all weights are equal;
    slot 7 of L is `unknown` (exactly 0 or 1), slot 7 of H is 0; guard cells are distance 0 and unknown; the record behind
    the grid is all zero.  2^-20 is the figure csrc/tdr_score_init.hip documents for the split."""
    pkg, k = tdr
    ref = S.reference(oracle, scene, "fixed", "plain", kind, 2.0 ** k2)
    m = _map(pkg, k, scene)
    with _Switches(k, 1, 0, 1):
        _search(pkg, k, m, ref, False)
    k.synchronize()
    sc, ncls = ref["sc"], ref["cfg"].ncls
    rows, cols = sc.class_mask.shape
    rec = m.dev.rec16.cpu().numpy().view(np.float16).astype(np.float64).reshape(-1, 2, 8)
    assert rec.shape[0] == (rows + 2) * (cols + 2) + 1
    assert not rec[-1].any(), "the record behind the grid"
    grid = rec[:-1].reshape(rows + 2, cols + 2, 2, 8)
    H, L = grid[:, :, 0], grid[:, :, 1]
    assert not H[:, :, 7].any()
    unknown = np.ones((rows + 2, cols + 2))
    unknown[1:-1, 1:-1] = sc.class_mask
    assert np.array_equal(L[:, :, 7], unknown)
    guard = np.ones((rows + 2, cols + 2), bool)
    guard[1:-1, 1:-1] = False
    assert not H[guard].any() and not L[guard][:, :7].any()
    assert not H[:, :, ncls:7].any() and not L[:, :, ncls:7].any()
    wc = np.asarray([np.float32(0.01 * float(np.float32(w))) for w in ref["params"]["class_weights"]], np.float32)
    if kind == "unit":
        fac = np.ones(ncls)
    else:
        e = 1 - int(np.frexp(float(wc.max()))[1])             # max * 2^e in [1, 2)
        fac = np.ldexp(wc.astype(np.float64), e)
        assert 1 <= fac.max() < 2
    worst = 0.0
    for c in range(ncls):
        want = fac[c] * sc.class_maps[c].astype(np.float64)
        got = (H[:, :, c] + L[:, :, c])[1:-1, 1:-1]
        pos = want > 0
        assert pos.any() and not got[~pos].any()
        worst = max(worst, float((np.abs(got[pos] - want[pos]) / want[pos]).max()))
    print(f"{scene} {kind} 2^{k2}: largest relative error of hi + lo {worst:.3e} (2^-20 = {2.0 ** -20:.3e})")
    assert worst <= 2.0 ** -20


# ---- the batched twins -------------------------------------------------------------------------------------------------------
def test_batched_search_chooses_exactly_pass_by_pass(tdr, oracle):
    """One tdr_batch_step with batch_init_search over three filters of 100 / 200 / 200 particles and rec16_min = 128: the
    first splits on the fly, the others take half records — two weight vectors, two sets of them — and the third's scan holds
    a count of 2049, which sends IT alone back to the vector kernel.  Every filter against the exact costs (a twin handle
    taken through the same propagate gives the states the search saw, and its standalone search must give the same bits);
    the counters sum over the filters."""
    from top_down_renderer_amd import batch
    pkg, k = tdr
    cfg, sc = S.scene(S.BATCH_SCENE)
    ncls, nb, nr = cfg.ncls, cfg.nb, cfg.nr
    mh = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    mh.sample_pts_polar(nb, nr, float(cfg.ang_res))
    prior = (0.4, 0.1, 0.01)
    st_all = S.states(S.BATCH_SCENE, "fixed")
    stepped, twins, refs, scans = [], [], [], []
    with _Switches(k, 1, S.BATCH_REC16_MIN, 1):
        try:
            batch.set_init_search_in_batch(True)
            for i, (n, kind, var) in enumerate(S.BATCH):
                pr = S.params(ncls, "fixed", kind)
                fp = pkg.FilterParams(**pr).to_c(ncls)
                pair = []
                for _ in range(2):
                    f = batch.FilterHandle(mh, n, fp, seed=31 + i)
                    f.set_states(st_all[:n])
                    pair.append(f)
                stepped.append(pair[0])
                twins.append(pair[1])
                pair[1].propagate(*prior)
                pre = pair[1].states()
                assert np.array_equal(pre["have_init"], st_all["have_init"][:n])
                refs.append(S.reference(oracle, S.BATCH_SCENE, "fixed", var, kind, 1.0, st=pre))
                scans.append(np.ascontiguousarray(refs[-1]["scan"].reshape(ncls, nr, nb).transpose(0, 2, 1)))
            got, v = counted(k, lambda: batch.step_batch(stepped, scans, float(cfg.res), [prior] * len(stepped)))
            assert got == (len(stepped), 0), got
            # the twins: the standalone search on the same states, no resample
            for f, s in zip(twins, scans):
                f.compute_weights(s, float(cfg.res))
        finally:
            batch.set_init_search_in_batch(False)
    print(f"batched: pass counters [12..15] = {v[12:]}")
    b = [r["search"].wanted_batches() for r in refs]
    assert b == [1, 3, 3]
    assert v[12:] == [b[1] + b[2], b[0], 0, b[2]], v
    for i, (fb, ft, ref) in enumerate(zip(stepped, twins, refs)):
        n, se = S.BATCH[i][0], ref["search"]
        post = ft.states()
        raw_t = ft.raw_weights(n)
        worst = _check_against_exact(oracle, ref, post["theta"].copy(), post["have_init"].copy(), raw_t)
        # the batched filter: its raw weights are the twin's; its states are the searched ones drawn by the resample
        raw_b = fb.raw_weights(n)
        assert np.array_equal(raw_b.view(np.uint32), raw_t.view(np.uint32))
        idx, stb = fb.resample_indices(), fb.states()
        assert np.array_equal(stb.view(np.uint8), post[idx].view(np.uint8))
        theta, have = ref["st"]["theta"].copy(), ref["st"]["have_init"].copy()
        theta[idx], have[idx] = stb["theta"], stb["have_init"]
        drawn = np.unique(idx)
        assert len(np.intersect1d(drawn, se.searched())) >= 10
        worst_b = X.check_choice(se, ref["st"]["theta"], theta, have, raw_b, ref["raw_o"], ref["st"]["have_init"], only=drawn)
        print(f"batched filter {i}: largest excess {max(worst, worst_b):.3e}")
