"""CPU-only: the NumPy restatement of map fusion (tests/fuse_ref.py) held to hand-worked facts, to the adjoint identity
against the oracle's gather, to the label rule's edges and to the closed loop the GPU test repeats; and what the library
refuses without touching a device."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import fuse_ref as FR
from oracle import np_oracle as no
from top_down_renderer_amd import _lib
from top_down_renderer_amd._lib import MapDescC

F32 = np.float32
vp = C.c_void_p


# ---- 1. a 5 x 5 map and a 4 x 2 polar scan, by hand ---------------------------------------------------------------------------
def test_hand_worked_5x5_map_4x2_scan():
    """nb = 4, nr = 2, ang_res = pi / 2: window rows look along -135, -45, +45, +135 degrees, ring 0 is the centre, ring 1
    has radius 1 * res = 1.5 cells: cos / sin of 45 degrees * 1.5 = 1.06 -> one cell diagonally.  Centre (cx, cy) = (2, 2):
    ring 1 of rows 0..3 = cells (row, col) (1, 1), (3, 1), (3, 3), (1, 3)."""
    nb, nr = 4, 2
    tab = no.polar_table(nb, nr, F32(np.pi / 2), 1.0)
    scan = np.zeros((2, nb * nr), F32)
    scan[0, 0 + nb * 0] = 5        # ring 0, row 0, class 0
    scan[1, 2 + nb * 0] = 7        # ring 0, row 2, class 1: the same centre cell
    scan[0, 0 + nb * 1] = 1        # ring 1, rows 0..3, class 0: 1, 2, 3, 4
    scan[0, 1 + nb * 1] = 2
    scan[0, 2 + nb * 1] = 3
    scan[0, 3 + nb * 1] = 4
    votes = np.zeros((2, 5, 5), np.uint32)
    added, dropped = FR.add_votes(votes, scan, FR.polar_cells(tab, nb, nr, 1.0, 5, 5, 2.0, 2.0, 0.0, 1.0, 1.5))
    want = np.zeros((2, 5, 5), np.uint32)
    want[0, 2, 2], want[1, 2, 2] = 5, 7
    want[0, 1, 1], want[0, 3, 1], want[0, 3, 3], want[0, 1, 3] = 1, 2, 3, 4
    assert np.array_equal(votes, want) and (added, dropped) == (22, 0)
    # theta = pi / 2 is a shift of one row: scan row i pairs with window row i - 1, so every ring-1 count moves on by one
    votes[:] = 0
    FR.add_votes(votes, scan, FR.polar_cells(tab, nb, nr, 1.0, 5, 5, 2.0, 2.0, np.pi / 2, 1.0, 1.5))
    want[0, 1, 1], want[0, 3, 1], want[0, 3, 3], want[0, 1, 3] = 2, 3, 4, 1
    assert np.array_equal(votes, want)
    # centre (cx, cy) = (0, 2), column 0: rows 0 and 1 look towards column -1 and are dropped (counts 1 + 2)
    votes[:] = 0
    added, dropped = FR.add_votes(votes, scan, FR.polar_cells(tab, nb, nr, 1.0, 5, 5, 0.0, 2.0, 0.0, 1.0, 1.5))
    assert (added, dropped) == (19, 3) and votes[0, 3, 1] == 3 and votes[0, 1, 1] == 4 and votes[0, 2, 0] == 5
    # scale 2 doubles the radius: 2.12 -> two cells diagonally
    votes[:] = 0
    FR.add_votes(votes, scan, FR.polar_cells(tab, nb, nr, 1.0, 5, 5, 2.0, 2.0, 0.0, 2.0, 1.5))
    assert votes[0, 0, 0] == 1 and votes[0, 4, 0] == 2 and votes[0, 4, 4] == 3 and votes[0, 0, 4] == 4


def test_counts_conversion():
    v = np.asarray([np.nan, -1, 0, 0.5, 0.99999994, 1, 2.75, 2.0 ** 31 - 128, 2.0 ** 31, np.inf], F32)
    assert FR.counts(v).tolist() == [0, 0, 0, 0, 0, 1, 2, 2 ** 31 - 128, 0, 0]


# ---- 2. the shift pairing where theta * nb / 2 pi sits on .5 --------------------------------------------------------------------
def test_shift_pairing_on_both_sides_of_a_half():
    nb, nr = 16, 3
    tab = no.polar_table(nb, nr, F32(2 * np.pi / nb), 1.0)
    rng = np.random.default_rng(3)
    scan = rng.integers(0, 4, (2, nb * nr)).astype(F32)
    t = F32(2.5 * 2 * np.pi / nb)
    around = [np.nextafter(t, F32(0)), t, np.nextafter(t, F32(10))]
    shifts = [no.rot_shift(x, nb) for x in around]
    assert shifts[0] == 2 and shifts[-1] == 3                # the boundary lies inside these three floats
    unshifted = FR.polar_cells(tab, nb, nr, 1.0, 40, 40, 20.0, 19.0, 0.0, 1.0, 4.0)
    for x, s in zip(around, shifts):
        got = np.zeros((2, 40, 40), np.uint32)
        FR.add_votes(got, scan, FR.polar_cells(tab, nb, nr, 1.0, 40, 40, 20.0, 19.0, x, 1.0, 4.0))
        # by hand: scan row i takes the cell of window row i - s
        rolled = np.roll(scan.reshape(2, nr, nb), -s, axis=2).reshape(2, nb * nr)
        want = np.zeros((2, 40, 40), np.uint32)
        FR.add_votes(want, rolled, unshifted)
        assert np.array_equal(got, want), (x, s)
    for x, s in ((-0.1, 0), (-0.3, nb - 1), (2 * np.pi + 0.5, 1)):    # negative and beyond 2 pi
        assert no.rot_shift(x, nb) == s


# ---- 3. the vote step is the transpose of the gather ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_adjoint_identity_against_the_oracle_gather(seed):
    """sum_c sum_cells V_c * M_c == sum_c sum_bins S_c(i, j) * L_c((i - s) mod nb, j), every product exact in double."""
    rng = np.random.default_rng(seed)
    ncls, H, W, nb, nr = 3, 37 + seed, 45 - seed, 20, 9
    resolution = [1.0, 2.0, 1.0][seed]
    maps = rng.uniform(0, 50, (ncls, H, W)).astype(F32)
    mask = (rng.random((H, W)) < 0.2).astype(np.uint8)
    tab = no.polar_table(nb, nr, F32(2 * np.pi / nb), resolution)
    for cx, cy, th, scale, res in ((20.0, 18.0, 0.7, 1.0, 2.0), (3.0, 60.0, -2.0, 1.3, 3.0), (-4.5, 10.0, 5.1, 0.8, 1.5)):
        scan = rng.integers(0, 6, (ncls, nb * nr)).astype(F32)
        votes = np.zeros((ncls, H, W), np.uint32)
        added, dropped = FR.add_votes(votes, scan, FR.polar_cells(tab, nb, nr, resolution, H, W, cx, cy, th, scale, res))
        assert dropped > 0 or (cx, cy) == (20.0, 18.0)       # the poses are partly off the map
        L, _ = no.local_map_polar(maps, mask, resolution, tab, cx, cy, scale, res)
        s = no.rot_shift(th, nb)
        b = np.arange(nb * nr)
        k = (b % nb - s) % nb + nb * (b // nb)
        lhs = math.fsum((votes.astype(np.float64) * maps.astype(np.float64)).ravel())
        rhs = math.fsum((scan.astype(np.float64) * L[:, k].astype(np.float64)).ravel())
        assert lhs == rhs and lhs > 0
        fl = sum(Fraction(int(v)) * Fraction(float(m)) for v, m in zip(votes.ravel(), maps.ravel()) if v)
        fr = sum(Fraction(float(x)) * Fraction(float(y)) for x, y in zip(scan.ravel(), L[:, k].ravel()) if x)
        assert fl == fr and Fraction(lhs) == fl               # (no product or sum above was rounded)


# ---- 4. the label rule ----------------------------------------------------------------------------------------------------------
def test_label_rule_edges():
    base = np.full((1, 8), 9, np.uint8)                       # one map row of 8 cells at resolution 1, base label 9
    cl = np.asarray([10, 11, 12], np.uint8)
    v = np.zeros((3, 1, 8), np.uint32)
    v[:, 0, 0] = (4, 4, 1)            # tie -> the lowest class; share 4/9 < 1/2 -> no verdict at 1/2, verdict at 4/9
    v[:, 0, 1] = (0, 5, 0)            # min_votes exactly met
    v[:, 0, 2] = (0, 4, 0)            # one short
    v[:, 0, 3] = (0, 6, 3)            # share 2/3 exactly met
    v[:, 0, 4] = (0, 5, 3)            # 5/8 < 2/3: one vote short
    v[:, 0, 5] = (2 ** 32 - 1, 0, 2 ** 31 - 1)   # products past 2^32 (and past 2^53 with den = 2^24)
    v[:, 0, 6] = (0, 0, 0)            # nothing
    v[:, 0, 7] = (1, 2 ** 32 - 2, 2 ** 32 - 1)
    assert FR.fuse_labels(v, base, cl, 5, 2, 3, 1.0)[0].tolist() == [9, 11, 9, 11, 9, 10, 9, 9]
    assert FR.fuse_labels(v, base, cl, 5, 4, 9, 1.0)[0].tolist() == [10, 11, 9, 11, 11, 10, 9, 12]
    # 2^24 as the denominator: (2^32 - 1) * 2^24 against (2^32 - 1 + 2^31 - 1) * num, decided exactly
    total = 2 ** 32 - 1 + 2 ** 31 - 1
    num = (2 ** 32 - 1) * 2 ** 24 // total                    # the largest numerator that still gives a verdict
    assert FR.fuse_labels(v, base, cl, 1, num, 2 ** 24, 1.0)[0, 5] == 10
    assert FR.fuse_labels(v, base, cl, 1, num + 1, 2 ** 24, 1.0)[0, 5] == 9
    # no verdict -> the BASE label, whatever an earlier result was: a pure function of (votes, base)
    assert FR.fuse_labels(np.zeros_like(v), base, cl, 1, 0, 1, 1.0).tolist() == base.tolist()


# ---- 5. the pixel of a cell -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,h,w", [(1.0, 9, 7), (2.0, 9, 7), (2.0, 11, 13)])
def test_the_pixel_of_a_cell_is_the_one_the_ingest_samples(res, h, w):
    ncls = 3
    lut = np.full(256, -1, np.int32)
    lut[:ncls] = np.arange(ncls)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 2, (h, w)).astype(np.uint8)
    iy, ix = FR.cell_pixels(h, w, res)
    rows, cols = len(iy), len(ix)
    assert (rows, cols) == (int(h / res), int(w / res))
    assert len(set(iy.tolist())) == rows and len(set(ix.tolist())) == cols      # one to one from resolution 1 on
    m0, k0 = no.load_compressed_raster_map(img, lut, ncls, res)
    for yi, xi in ((0, 0), (rows - 1, cols - 1), (rows // 2, 1)):
        b = img.copy()
        b[iy[yi], ix[xi]] = 2                                                  # a class no other pixel holds
        m1, _ = no.load_compressed_raster_map(b, lut, ncls, res)
        inside = m1[2] == 0                                                    # the cells of class 2
        assert inside.sum() == 1 and inside[yi, xi]
        # ... and through fuse_labels: a verdict for class 2 in that cell alone writes that pixel alone
        v = np.zeros((ncls, rows, cols), np.uint32)
        v[2, yi, xi] = 3
        assert np.array_equal(FR.fuse_labels(v, img, np.arange(ncls, dtype=np.uint8), 1, 1, 1, res), b)
        assert FR.changed_cells(img, b, lut, ncls, res) == 1
    assert m0.shape == (ncls, rows, cols) and k0.shape == (rows, cols)


# ---- 6. the closed loop ---------------------------------------------------------------------------------------------------------
def test_closed_loop_lowers_the_cost_at_every_true_pose():
    sc = FR.closed_loop_scene()
    votes, fused = FR.closed_loop_fuse(sc)
    assert (fused != sc["base_img"]).any()
    y0, y1, x0, x1 = sc["block"]
    block = np.zeros((sc["size"], sc["size"]), bool)
    block[y0:y1, x0:x1] = True
    fixed = (fused == sc["true_img"])[::-1][block].mean()
    assert fixed > 0.5, fixed                                  # most of the mislabelled block is put right
    stale = no.load_compressed_raster_map(sc["base_img"], sc["lut"], sc["ncls"], 1.0)
    fresh = no.load_compressed_raster_map(fused, sc["lut"], sc["ncls"], 1.0)
    for k in range(len(sc["poses"])):
        before, after = FR.pose_cost(*stale, sc, k), FR.pose_cost(*fresh, sc, k)
        assert after < before, (k, before, after)


# ---- 7. refused without a device -------------------------------------------------------------------------------------------------
def test_refusals_need_no_device():
    L = _lib.load()
    h = vp()
    cl = np.arange(3, dtype=np.uint8)
    a, d = C.c_uint64(7), C.c_uint64(7)
    ch, kept = C.c_int64(7), C.c_int(7)
    pose = np.asarray([1, 1, 0, 1, 1], F32)
    img = np.zeros((3, 16), F32)
    assert L.tdr_fuser_create(None, cl.ctypes.data_as(vp), 1, 1, 2, C.byref(h)) == -1
    assert "null pointer" in L.tdr_last_error().decode() and not h.value
    assert L.tdr_fuser_add(None, None, 1, 1, 0, 1, 1, C.byref(a), C.byref(d)) == -1
    assert L.tdr_fuser_add_batch(None, None, 1, pose.ctypes.data_as(vp), C.byref(a), C.byref(d)) == -1
    assert L.tdr_fuser_add_images(None, img.ctypes.data_as(vp), 1, 4, 4, 1, 1, 0, 1, 1, C.byref(a), C.byref(d)) == -1
    assert L.tdr_fuser_apply(None, None, 0, C.byref(ch)) == -1
    assert L.tdr_fuser_decay(None, 1) == -1 and L.tdr_fuser_reset(None) == -1
    assert L.tdr_fuser_rebase(None, C.byref(kept)) == -1
    assert L.tdr_fuser_get_votes(None, None) == -1 and L.tdr_fuser_get_labels(None, None) == -1
    assert L.tdr_fuser_stats(None, None) == -1
    assert (a.value, d.value, ch.value, kept.value) == (7, 7, 7, 7)
    L.tdr_fuser_destroy(None)
    # the launchers check their arguments before any launch
    desc = MapDescC()
    desc.ncls, desc.rows, desc.cols, desc.rec_floats, desc.resolution = 3, 10, 10, 4, 1.0
    p = vp(8)
    assert L.tdr_k_fuse_votes_jobs(C.byref(desc), None, 0, 0, None, 1, 16, p, p, p, None) == -1
    assert L.tdr_k_fuse_votes_jobs(C.byref(desc), None, 0, 0, p, 0, 16, p, p, p, None) == -1
    assert L.tdr_k_fuse_votes_jobs(C.byref(desc), None, 4, 4, p, 1, 16, p, p, p, None) == -1       # a shape, no table
    assert L.tdr_k_fuse_votes(C.byref(desc), None, 0, 0, p, 1, 4, 4, 1, 1, 0, 1, 1, p, p, p, None) == -1   # polar, no table
    assert L.tdr_k_fuse_votes(C.byref(desc), p, 4, 4, p, 1, 4, 5, 1, 1, 0, 1, 1, p, p, p, None) == -1      # another shape
    assert "table" in L.tdr_last_error().decode()
    assert L.tdr_k_fuse_votes(C.byref(desc), None, 0, 0, p, 0, 0, 4, 1, 1, 0, 1, 1, p, p, p, None) == -1
    desc.resolution = 0.0
    assert L.tdr_k_fuse_votes(C.byref(desc), None, 0, 0, p, 0, 4, 4, 1, 1, 0, 1, 1, p, p, p, None) == -1
    lab = lambda res, mv, num, den, h=10, w=10: L.tdr_k_fuse_labels(   # noqa: E731
        p, 3, 10, 10, h, w, C.c_float(res), cl.ctypes.data_as(vp), mv, num, den, p, p, p, 1, p, None)
    assert lab(0.5, 1, 1, 2, 5, 5) == -1 and "resolution" in L.tdr_last_error().decode()
    assert lab(1.0, 0, 1, 2) == -1 and lab(1.0, 1, 3, 2) == -1 and lab(1.0, 1, 1, 0) == -1
    assert lab(1.0, 1, 1, 2, 11, 10) == -1                                      # the image is not the map's
    assert L.tdr_k_fuse_labels(p, 3, 10, 10, 10, 10, C.c_float(1.0), cl.ctypes.data_as(vp), 1, 1, 2, p, p, p, 2, p, None) == -1
    assert L.tdr_k_fuse_decay(None, 3, 10, 10, 1, p, None) == -1 and L.tdr_k_fuse_decay(p, 3, 10, 10, -1, p, None) == -1
