"""What the Cartesian heading search must give, from the CPU oracle as it is (shared by tests/test_cart_init.py and
tests/test_cart_filter.py; not a test module).

Candidates are the reference's float loop in NumPy; every candidate of every particle is scored by
oracle.compute_weights_cart; the first maximum of the weight with NaN skipped is the oracle's choice.  A different device
choice passes only if the oracle's weight at the device's heading is within TIE_RTOL (relative) of the oracle's maximum —
the tie rule and the number of test_init_search_c1; every mismatch is checked.  Weights at the chosen heading: within
WEIGHT_RTOL of the oracle, the project's Cartesian tolerance."""
import numpy as np

from top_down_renderer_amd import synth

TIE_RTOL = 2e-5
WEIGHT_RTOL = 1e-5
N_ALL = 200
CASES = {"c6_32x24": (6, 32, 24, 41), "c11_21x13": (11, 21, 13, 43)}   # classes, window rows, window cols, seed


def candidates():
    """`for (float t = 0; t < 2*M_PI; t += 2*M_PI/40)`: float t, double increment."""
    out, t = [], np.float32(0)
    while float(t) < 2 * np.pi:
        out.append(t)
        t = np.float32(float(t) + 2 * np.pi / 40)
    return np.asarray(out, np.float32)


def make_case(name):
    """A 300 x 260 synth map, a Cartesian scan rendered from a pose on a road, and N_ALL particles around that pose:
    [0] far off the map (no finite candidate), [1] on the map's border, the rest scattered with their own scales."""
    ncls, rows, cols, seed = CASES[name]
    cfg = synth.Config(name, 5000, ncls, rows, cols, 300, N_ALL, polar=False, seed=seed, res=0.75)
    rng = np.random.default_rng(seed)
    lab = synth.make_label_image(300, ncls, rng)[:, :260].copy()
    maps, mask = synth.label_to_maps(lab, ncls)
    pose = synth.pick_true_pose(lab, rng, 60)
    pts = synth.make_scan(cfg, lab, pose, rng)
    st = synth.make_particles(cfg, lab, pose, rng, n=N_ALL, sigma_px=40.0, uniform_frac=0.2)
    st["scale"] = rng.uniform(0.8, 1.25, N_ALL).astype(np.float32)
    st["dx_m"] = rng.normal(0, 2, N_ALL).astype(np.float32)
    st["dy_m"] = rng.normal(0, 2, N_ALL).astype(np.float32)
    st["init_x_px"][0], st["init_y_px"][0] = -500.0, 150.0
    st["init_x_px"][1], st["init_y_px"][1] = 259.5, 0.5
    st["dx_m"][:2] = st["dy_m"][:2] = 0
    return cfg, lab, maps, mask, pose, pts, st


def oracle_candidate_weights(oracle, om, rows, cols, scan, res, fpo, st):
    """(len(st), 40) oracle weights: particle i at candidate heading j."""
    th = candidates()
    cand = np.repeat(st, len(th))
    cand["theta"] = np.tile(th, len(st))
    cand["have_init"] = 1
    with np.errstate(all="ignore"):
        w = oracle.compute_weights_cart(om, rows, cols, scan, res, fpo, np.ascontiguousarray(cand))
    return w.reshape(len(st), len(th))


def oracle_choice(w40):
    """First maximum of the weight per row, NaN skipped: (theta, index or -1)."""
    th = candidates()
    theta, idx = np.zeros(len(w40), np.float32), -np.ones(len(w40), np.int64)
    for i, row in enumerate(w40):
        best = 0.0
        for j, w in enumerate(row):
            if w > best:
                best, theta[i], idx[i] = w, th[j], j
    return theta, idx


def check_search(oracle, om, rows, cols, scan, res, fpo, st_in, w40, got_st, got_raw):
    """The launcher's outcome for the states st_in against the oracle (w40: candidate weights of st_in's rows)."""
    th = candidates()
    un = st_in["have_init"] == 0
    assert got_st["have_init"].all()
    for name in ("init_x_px", "init_y_px", "dx_m", "dy_m", "scale"):
        assert np.array_equal(got_st[name].view(np.uint32), st_in[name].view(np.uint32)), name
    # particles that had a heading keep it bit for bit
    assert np.array_equal(got_st["theta"][~un].view(np.uint32), st_in["theta"][~un].view(np.uint32))
    want_theta, want_idx = oracle_choice(w40)
    for i in np.nonzero(un)[0]:
        t = got_st["theta"][i]
        if t == want_theta[i]:
            continue
        j = np.nonzero(th == t)[0]
        assert len(j) == 1, f"particle {i}: theta {t!r} is not one of the candidates"
        assert want_idx[i] >= 0, f"particle {i}: no finite candidate, theta must be 0, got {t!r}"
        w_dev, w_best = w40[i, j[0]], w40[i, want_idx[i]]
        assert not np.isnan(w_dev), f"particle {i}: a NaN candidate was chosen"
        tie = abs(float(w_dev) - float(w_best)) / max(abs(float(w_best)), 1e-30)
        print(f"particle {i}: device chose candidate {j[0]}, oracle {want_idx[i]}, relative gap {tie:.3e}")
        assert tie <= TIE_RTOL, f"particle {i}: chosen heading is not a near-tie of the oracle's: {tie:.2e}"
    # the weights the regular launch gives at the chosen headings
    with np.errstate(all="ignore"):
        ref = oracle.compute_weights_cart(om, rows, cols, scan, res, fpo, np.ascontiguousarray(got_st))
    assert np.array_equal(np.isnan(got_raw), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(got_raw[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), 1e-30)
    print(f"max relative weight error {err.max(initial=0.0):.3e} over {int(ok.sum())} particles")
    assert err.max(initial=0.0) <= WEIGHT_RTOL
