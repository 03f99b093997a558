"""Scan bins that hold several classes in score_polar_su_kernel's assembly path (csrc/tdr_score_su.hip): with
tdr_config_tuning("su_full_list", 1) they are empty to the generated loop and a list pass behind it adds them, sector by
sector, from the class planes; with 0 the loop hands every four-ring step that holds one to the C++ step.  Integer sums:
every case demands the SAME BITS from (a) the list pass, (b) the hand-back and (c) the launch with every particle through
the ray-mapped kernel, the float kernel's weights to its rounding (3e-6, tests/test_shift_uniform.py), and the kernel's own
counters (tdr_profile_su_list, tdr_profile_variants): no hand-back with the list on and some with it off (where the scan
has such a bin), listed bins == dense waves x bins with several classes, nothing on the far path — the assembly path ran.
test_inputs_are_what_the_cases_say checks each case's scan and particles on the CPU.  Run with `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest

from test_shift_uniform import ALL_RAY, N_TOTAL, _assert_float_form_agrees, tdr  # noqa: F401

NB, NR, SIZE = 32, 16, 96
SHIFTS = ((0, 128), (1, 128), (NB - 1, 64))     # heading bin -> particles: 256 + 64 in one cloud, five waves


def _maps(ncls, holes):
    from top_down_renderer_amd import synth
    rng = np.random.default_rng(4100 + ncls)
    lab = synth.make_label_image(SIZE, ncls, rng)
    lab[lab < 0] = 0
    maps, _ = synth.label_to_maps(lab, ncls, 1.0)
    maps = maps.astype(np.float32).copy()
    mask = np.zeros((SIZE, SIZE), np.uint8)
    if holes:
        mask[1::3, 1::3] = 1
    maps[:, mask == 1] = 0
    return maps, mask


def _particles(where, scale_fixed=True):
    from top_down_renderer_amd import synth
    rng = np.random.default_rng(77)
    n = sum(c for _, c in SHIFTS)
    st = np.zeros(n, synth.STATE_DTYPE)
    st["scale"] = 1.0 if scale_fixed else rng.uniform(0.8, 1.2, n).astype(np.float32)
    st["have_init"] = 1
    at = 0
    for shift, c in SHIFTS:
        st["theta"][at:at + c] = np.float32(2 * np.pi * shift / NB)
        at += c
    centre = SIZE / 2 + 0.25 if where == "middle" else 1.25      # the corner: windows reach past two borders
    st["init_x_px"] = (centre + rng.normal(0.0, 1.5, n).clip(-4.0, 4.0)).astype(np.float32)
    st["init_y_px"] = (centre + rng.normal(0.0, 1.5, n).clip(-4.0, 4.0)).astype(np.float32)
    return st


def _single(rng, ncls):
    """(ncls, NB * NR), bin (scan row i, ring j) at i + NB * j: 45 % empty, every other bin one class, counts 1..5"""
    P = NB * NR
    scan = np.zeros((ncls, P), np.float32)
    full = rng.random(P) >= 0.45
    scan[rng.integers(0, ncls, P)[full], np.nonzero(full)[0]] = rng.integers(1, 6, int(full.sum())).astype(np.float32)
    return scan


def _add_class(scan, i, j, rng, classes=2, count=None):
    k = i + NB * j
    scan[:, k] = 0
    cls = rng.permutation(scan.shape[0])[:classes]
    scan[cls, k] = rng.integers(1, 6, classes).astype(np.float32)
    if count is not None:
        scan[cls[0], k] = np.float32(count)


def _scan(kind, ncls):
    rng = np.random.default_rng(500 + len(kind) + ncls)
    scan = _single(rng, ncls)
    if kind == "none":
        pass
    elif kind == "every":
        for k in range(NB * NR):
            _add_class(scan, k % NB, k // NB, rng)
    elif kind == "corners":   # first / last scan row of a sector (NB / 8 = 4 rows) x first / last ring of a group; rows NB - 1 and 0
        for i, j in ((0, 0), (NB // 8 - 1, NR - 1), (NB - 1, 5), (0, 9), (NB // 8, 4), (NB - 1, NR - 1)):
            _add_class(scan, i, j, rng)
    elif kind == "large":     # 2, 3 and all classes; one count of 2^23 (the mass bound stays below 2^24 x 256)
        _add_class(scan, 3, 2, rng, 2)
        _add_class(scan, 17, 7, rng, 3, count=1 << 23)
        _add_class(scan, 30, 13, rng, ncls)
    elif kind == "mixed":     # one bin in sixteen
        for k in rng.choice(NB * NR, NB * NR // 16, replace=False):
            _add_class(scan, int(k) % NB, int(k) // NB, rng, int(rng.integers(2, 4)))
    else:
        raise KeyError(kind)
    return scan


def n_full(scan):
    return int(((scan != 0).sum(axis=0) > 1).sum())


# case -> scan, classes, map with unknown cells, cloud, fixed scale, knobs
CASES = {
    "1 no such bin": dict(scan="none", ncls=6, holes=False, where="middle"),
    "2 every bin": dict(scan="every", ncls=6, holes=False, where="middle"),
    "3 sector and group corners, wrapping rows": dict(scan="corners", ncls=6, holes=False, where="middle"),
    "4 large counts": dict(scan="large", ncls=6, holes=False, where="middle"),
    "4 large counts, four classes": dict(scan="large", ncls=4, holes=False, where="middle"),
    "5 all known": dict(scan="mixed", ncls=6, holes=False, where="middle", variant=0),
    "5 unknown cells inside the box": dict(scan="mixed", ncls=6, holes=True, where="middle", variant=1),
    "5 map corner": dict(scan="mixed", ncls=6, holes=True, where="corner", variant=2),
    "6 groups of 4, tail units": dict(scan="mixed", ncls=6, holes=True, where="middle", su_group=4, tail=(2, 4)),
    "6 groups of 8, tail units": dict(scan="mixed", ncls=6, holes=True, where="middle", su_group=8, tail=(1, 8)),
    "6 groups of 16, tail units": dict(scan="mixed", ncls=6, holes=True, where="middle", su_group=16, tail=(1, 2)),
    "7 per-particle scale": dict(scan="mixed", ncls=6, holes=True, where="middle", scale_fixed=False),
}


def _inputs(case):
    c = CASES[case]
    maps, mask = _maps(c["ncls"], c["holes"])
    return c, maps, mask, _particles(c["where"], c.get("scale_fixed", True)), _scan(c["scan"], c["ncls"])


def _cells(oracle, st, i, j):
    """Map cell (row, column) of window sample (direction i, ring j) of every particle, as the kernels form it."""
    tab = oracle.polar_table(NB, NR, np.float32(2 * np.pi / NB))
    t = tab[i + NB * j].astype(np.float32)
    sc = st["scale"].astype(np.float32)
    cx = st["dx_m"] * sc + st["init_x_px"]
    cy = st["dy_m"] * sc + st["init_y_px"]
    r = np.clip((t[0] * sc) * np.float32(1.0) + cy, -1.0, SIZE).astype(np.float32)
    c = np.clip((t[1] * sc) * np.float32(1.0) + cx, -1.0, SIZE).astype(np.float32)
    return np.floor(r + np.float32(0.49999997)).astype(int), np.floor(c + np.float32(0.49999997)).astype(int)


@pytest.mark.parametrize("case", list(CASES))
def test_inputs_are_what_the_cases_say(oracle, case):
    c, maps, mask, st, scan = _inputs(case)
    P = NB * NR
    assert scan.shape == (c["ncls"], P) and len(st) == 256 + 64
    # an integer form: whole counts below 2^24, the mass bound of score_prep_kernel below 2^24
    assert (scan >= 0).all() and (scan == np.floor(scan)).all() and scan.max() < (1 << 24)
    tot = scan.sum(axis=0, dtype=np.float64)
    assert ((tot[tot >= 1].astype(np.int64) >> 8) + 1).sum() < (1 << 24)
    per_bin = (scan != 0).sum(axis=0)
    want = {"none": 0, "every": P, "corners": 6, "large": 3, "mixed": P // 16}[c["scan"]]
    assert n_full(scan) == want
    shifts = [oracle.rot_shift(float(t), NB) for t in st["theta"]]
    at = 0
    for shift, cnt in SHIFTS:
        assert set(shifts[at:at + cnt]) == {shift}
        at += cnt
    if c["scan"] == "corners":
        # a sector is NB / 8 directions i0 .. i0 + 3, paired with scan rows (i + shift) mod NB: for shifts 1 and NB - 1 one
        # sector's rows run over NB - 1 into 0, and the bins in rows NB - 1 and 0 sit on either side of that wrap
        for shift in (1, NB - 1):
            rows = [[(i + shift) % NB for i in range(s * (NB // 8), (s + 1) * (NB // 8))] for s in range(8)]
            assert any(NB - 1 in r and 0 in r and r[0] != 0 for r in rows)
        assert per_bin[0 + NB * 0] == 2 and per_bin[NB // 8 - 1 + NB * (NR - 1)] == 2 and per_bin[NB - 1 + NB * 5] == 2 and per_bin[NB * 9] == 2
    if c["scan"] == "large":
        assert sorted(per_bin[per_bin > 1]) == [2, 3, c["ncls"]] and scan.max() == float(1 << 23)
    variant = c.get("variant")
    if variant is not None:
        # a bin with several classes whose cell is: known for every lane / known for some lanes and unknown for others /
        # clamped into the guard ring (outside the map) for some lanes
        hit_mixed = hit_clamp = False
        for k in np.nonzero(per_bin > 1)[0]:
            r_scan, j = int(k) % NB, int(k) // NB
            at = 0
            for shift, cnt in SHIFTS:
                ri, ci = _cells(oracle, st[at:at + cnt], (r_scan - shift) % NB, j)
                at += cnt
                outside = (ri < 0) | (ri >= SIZE) | (ci < 0) | (ci >= SIZE)
                known = ~outside & (mask[ri.clip(0, SIZE - 1), ci.clip(0, SIZE - 1)] == 0)
                if variant == 0:
                    assert known.all()
                hit_mixed |= bool(known.any() and not known.all() and not outside.any())
                hit_clamp |= bool(outside.any())
        assert variant != 1 or hit_mixed
        assert variant != 2 or hit_clamp


def _knob(k, name, v):
    assert k.lib.tdr_config_tuning(name.encode(), int(v)) >= 0, name


class _Launch:
    """One filter on one map and scan; run(span, full_list) -> raw weights of the integer form."""

    def __init__(self, pkg, k, c, maps, mask, st, scan):
        import torch
        self.k, self.n = k, len(st)
        self.m = pkg.TopDownMapPolar(pkg.Params(resolution=1.0), maps, mask, kernels=k)
        assert self.m.dev.desc.cwords > 0
        self.m.samplePtsPolar((NB, NR), np.float32(2 * np.pi / NB))
        self.pk = self.m.scan_handle(scan)
        self.f = pkg.ParticleFilter(self.n, self.m, pkg.FilterParams(fixed_scale=1.0 if c.get("scale_fixed", True) else -1.0),
                                    kernels=k, init_particles=False, locality_every=1)
        self.f.set_states(st)
        self.perm = k.zeros((self.f.cap_local,), torch.int32)
        k.locality_order(self.f.st, self.n, self.m.rows, self.m.cols, self.perm)

    def run(self, span, full_list=1, mode=2):
        k, f = self.k, self.f
        k.lib.tdr_config_shift_uniform(mode)
        k.lib.tdr_config_shift_uniform_span(span)
        _knob(k, "su_full_list", full_list)
        f.raw_w.fill_(-7.0)
        k.score(self.m.dev, self.pk, 1.0, f.fp_c, f.st, self.n, f.raw_w, perm=self.perm, uniform_scale=f._uniform_scale,
                n_total=N_TOTAL)
        k.synchronize()
        return f.raw_w[:self.n].cpu().numpy()

    def counted(self, full_list):
        """(weights, steps handed back, bins listed, the 16 variant counters) of an all-dense launch"""
        k = self.k
        v, w = (C.c_int64 * 16)(), (C.c_int64 * 2)()
        try:
            k.lib.tdr_profile_enable(2)
            assert k.lib.tdr_profile_variants(v) == 0 and k.lib.tdr_profile_su_list(w) == 0    # (reading resets)
            raw = self.run(0.0, full_list)
            assert k.lib.tdr_profile_variants(v) == 0 and k.lib.tdr_profile_su_list(w) == 0
        finally:
            k.lib.tdr_profile_enable(0)
        return raw, int(w[0]), int(w[1]), [int(x) for x in v]


@pytest.fixture()
def restore(tdr):
    _, k = tdr
    names = ("su_tail_groups", "su_tail_parts", "su_group", "su_full_list")
    before = {n: int(k.lib.tdr_config_tuning(n.encode(), -1)) for n in names}
    mode = k.lib.tdr_config_shift_uniform(-1)
    yield
    for n, v in before.items():
        _knob(k, n, v)
    k.lib.tdr_config_shift_uniform(mode)
    k.lib.tdr_config_shift_uniform_span(-2.0)
    k.lib.tdr_profile_enable(0)


WAVES = sum((c + 63) // 64 for _, c in SHIFTS)   # dense waves of an all-dense launch: every heading bin padded to whole waves


def _check(case, L, scan, variant=None):
    nf = n_full(scan)
    on, hand_on, listed_on, v_on = L.counted(1)
    off, hand_off, listed_off, v_off = L.counted(0)
    print(f"{case}: several-class bins {nf}; list on: handed back {hand_on}, listed {listed_on}, variants {v_on[:7]}; "
          f"list off: handed back {hand_off}, listed {listed_off}")
    assert not (on == -7.0).any()
    assert np.array_equal(on, off, equal_nan=True), "list pass != hand-back"
    assert np.array_equal(on, L.run(0.0, 1), equal_nan=True), "counting changed the weights"
    assert np.array_equal(on, L.run(ALL_RAY, 1), equal_nan=True), "list pass != ray-mapped kernel"
    _assert_float_form_agrees(L.run(0.0, 1, mode=0), on)
    assert v_on[6] == 0 and v_off[6] == 0, "a wave took the far path"
    assert sum(v_on[:6]) > 0
    assert hand_on == 0 and listed_off == 0
    assert listed_on == WAVES * nf
    assert (hand_off > 0) == (nf > 0)
    if variant is not None:   # the loop variant the case is for ran ([0..2] / [3..5]: all known, inside, general)
        assert v_on[variant] + v_on[3 + variant] > 0, v_on[:7]
    return on


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_list_pass_equals_hand_back_and_ray_kernel(tdr, oracle, restore, case):
    pkg, k = tdr
    c, maps, mask, st, scan = _inputs(case)
    if "su_group" in c:
        _knob(k, "su_group", c["su_group"])
        _knob(k, "su_tail_groups", c["tail"][0])
        _knob(k, "su_tail_parts", c["tail"][1])
    L = _Launch(pkg, k, c, maps, mask, st, scan)
    raw = _check(case, L, scan, c.get("variant"))
    # ... and the oracle, to 1e-5 like every scoring test
    ref = oracle.compute_weights(oracle.OracleMap(maps, mask, 1.0), oracle.polar_table(NB, NR, np.float32(2 * np.pi / NB)), NB, NR,
                                 scan, 1.0, oracle.make_params(c["ncls"], fixed_scale=1.0 if c.get("scale_fixed", True) else -1.0),
                                 st.copy())
    assert np.array_equal(np.isnan(raw), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert (np.abs(raw[ok] - ref[ok]) <= 1e-5 * np.abs(ref[ok])).all()


@pytest.mark.gpu
def test_the_preparation_writes_the_mask_twice_over(tdr, restore):
    """The new product of score_prep_kernel, out of the workspace the preparation ran on: word (group, scan row) has bit jj
    set where bin (row, group * G + jj) holds several classes, and the rows are stored twice."""
    import torch
    from top_down_renderer_amd.kernels import _ptr
    pkg, k = tdr
    c, maps, mask, st, scan = _inputs("5 unknown cells inside the box")
    several = ((scan != 0).sum(axis=0) > 1).reshape(NR, NB)     # [ring][scan row]
    k.lib.tdr_config_shift_uniform(2)
    for G in (4, 8, 16):
        _knob(k, "su_group", G)
        L = _Launch(pkg, k, c, maps, mask, st, scan)
        ws = k.zeros((int(k.lib.tdr_score_workspace_floats(c["ncls"], NB, NR, L.n, N_TOTAL)),), torch.float32)
        lay, _ = k.score_prep(L.m.dev, L.pk, 1.0, L.f.st, L.n, perm=L.perm, uniform_scale=1.0, n_total=N_TOTAL, span=0.0, workspace=ws)
        words = C.c_int64(0)
        assert k.lib.tdr_k_score_prep_full_mask(C.byref(L.m.dev.desc), NB, NR, L.n, N_TOTAL, None, None, C.byref(words), None) == 0
        assert lay[0] == G and words.value == (NR // G) * 2 * NB
        got = k.zeros((words.value,), torch.int32)
        assert k.lib.tdr_k_score_prep_full_mask(C.byref(L.m.dev.desc), NB, NR, L.n, N_TOTAL, _ptr(ws), _ptr(got), C.byref(words),
                                                k.stream()) == 0
        k.synchronize()
        got = got.cpu().numpy().view(np.uint32).reshape(NR // G, 2, NB)
        want = np.zeros((NR // G, NB), np.uint32)
        for j in range(NR):
            want[j // G] |= several[j].astype(np.uint32) << np.uint32(j % G)
        assert want.any()
        assert np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want)


@pytest.mark.gpu
def test_one_batched_step_equals_the_standalone_one(tdr, restore):
    """Case 8: two filters stepped by tdr_batch_step on one map end on the bits of the filter stepped alone, on the scan with
    several-class bins, list pass on and off — and both settings agree.  (tdr_batch_step batches the float form only: filters
    whose launch has an integer form run their standalone calls inside it, which is what the assertion on its statistics
    says.)"""
    pkg, k = tdr
    from top_down_renderer_amd import batch
    c, maps, mask, st, scan = _inputs("5 unknown cells inside the box")
    imgs = np.ascontiguousarray(scan.reshape(c["ncls"], NR, NB).transpose(0, 2, 1))   # (ncls, nb, nr)
    k.lib.tdr_config_shift_uniform(2)
    m = batch.MapHandle(maps, mask, resolution=1.0)
    m.sample_pts_polar(NB, NR, np.float32(2 * np.pi / NB))
    n = len(st)

    def make(seed):
        f = batch.FilterHandle(m, n, pkg.FilterParams(fixed_scale=1.0), seed=seed)
        f.configure(1)
        f.set_states(st)
        return f

    got = {}
    for full_list in (1, 0):
        _knob(k, "su_full_list", full_list)
        alone = make(3)
        alone.propagate(0.5, 0.0, 0.01)
        alone.update(imgs, 1.0)
        pair = [make(3), make(3)]
        batched, standalone = batch.step_batch(pair, [imgs, imgs], 1.0, [(0.5, 0.0, 0.01)] * 2)
        assert (batched, standalone) == (0, 2)    # (an integer-form filter runs its standalone calls inside the batch)
        got[full_list] = alone.raw_weights(n)
        assert np.isfinite(got[full_list]).any()
        for f in pair:
            assert np.array_equal(f.raw_weights(n), got[full_list], equal_nan=True)
    assert np.array_equal(got[0], got[1], equal_nan=True)
