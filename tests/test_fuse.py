"""GPU: map fusion (csrc/tdr_fuse.hip, csrc/tdr_host_fuse.cpp; include/tdr.h, "map fusion") against its NumPy restatement
(tests/fuse_ref.py), byte for byte: the vote scatter through the handle, the launchers and the Python class; the label pass
and apply against a map built fresh from the fused image; decay, reset, rebase; the closed loop; what is refused.
Shapes are chosen for where the kernels can go wrong (ragged edge tiles, several blocks, every class count's record size),
not for the workload."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fuse_ref as FR
from oracle import np_oracle as no

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
pytestmark = pytest.mark.gpu
F32 = np.float32
vp = C.c_void_p
UNKNOWN = 200
MAPS = {"96x80r1": (96, 80, 1.0), "97x81r2": (97, 81, 2.0)}      # image rows x cols, resolution
POLAR = [(16, 9), (100, 25)]
WINDOWS = [(1, 1), (7, 5), (33, 32)]


def _lut(ncls):
    lut = np.full(256, -1, np.int32)
    lut[:ncls] = np.arange(ncls)
    return lut


def _image(rng, h, w, ncls):
    img = rng.integers(0, ncls, (h, w)).astype(np.uint8)
    img[rng.random((h, w)) < 0.1] = UNKNOWN
    return img


def _scan(rng, ncls, P, hi=6):
    s = rng.integers(1, hi, (ncls, P)).astype(F32)
    s[rng.random((ncls, P)) < 0.7] = 0
    return s


def _imgs(scan, rows, cols):
    """(ncls, P) in the render layout (bin i + rows * j) -> the (ncls, rows, cols) images add_images takes"""
    return np.ascontiguousarray(scan.reshape(scan.shape[0], cols, rows).transpose(0, 2, 1))


def _make_map(img, ncls, res, center=(0, 0)):
    from top_down_renderer_amd import batch
    return batch.MapHandle.from_labels(img, _lut(ncls), ncls, res, center)


def _set_labels(m, img, ncls, res, center=(0, 0)):
    from top_down_renderer_amd._lib import check
    lut = _lut(ncls)
    img = np.ascontiguousarray(img, np.uint8)
    check(m.L.tdr_map_set_labels(m.h, img.ctypes.data_as(vp), img.shape[0], img.shape[1], lut.ctypes.data_as(vp), 256, ncls,
                                 C.c_float(res), center[0], center[1]))


_hip = None


def _read(ptr, nbytes):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    out = np.zeros(nbytes, np.uint8)
    assert _hip.hipDeviceSynchronize() == 0
    assert _hip.hipMemcpy(out.ctypes.data_as(vp), vp(ptr), C.c_size_t(nbytes), 2) == 0
    return out


def _records(m):
    """the map's dense records and, decoded on the device, its class maps and mask (tdr_map_get_desc + tdr_k_unpack_map)"""
    import torch
    from top_down_renderer_amd._lib import MapDescC, check
    d = MapDescC()
    check(m.L.tdr_map_get_desc(m.h, C.byref(d)))
    rec = _read(d.rec, 4 * int(m.L.tdr_map_rec_floats_total(d.ncls, d.rows, d.cols)))
    maps = torch.empty((d.ncls, d.cols, d.rows), dtype=torch.float32, device="cuda")
    mask = torch.empty((d.cols, d.rows), dtype=torch.uint8, device="cuda")
    check(m.L.tdr_k_unpack_map(vp(d.rec), d.ncls, d.rows, d.cols, vp(maps.data_ptr()), vp(mask.data_ptr()), None))
    torch.cuda.synchronize()
    return rec, maps.cpu().numpy().transpose(0, 2, 1).copy(), mask.cpu().numpy().T.copy(), (d.cwords, d.dict_n)


def _poses(rows, cols, res):
    """(cx, cy) in the units tdr_k_local_map_* takes (cells * resolution): mid-map, straddling each edge, wholly off"""
    w, h = cols * res, rows * res
    return [(0.5 * w, 0.5 * h), (0.6, 0.4 * h), (w - 0.7, 0.3 * h), (0.45 * w, 0.3), (0.4 * w, h - 0.6), (-50.0 * w, 0.5 * h)]


def _boundary(nb):
    t = F32(2.5 * 2 * np.pi / nb)
    return [float(np.nextafter(t, F32(0))), float(t), float(np.nextafter(t, F32(10)))]


@pytest.fixture(scope="module")
def oracle_mod(oracle):
    return oracle


# ---- votes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [1, 6, 15])
@pytest.mark.parametrize("mapname", list(MAPS))
def test_votes_are_byte_equal_to_the_restatement(mapname, ncls, oracle_mod):
    """The launchers (one scan per launch; only the map's shape and resolution are read, so the records are a dummy):
    votes, counters and the dirty bitmap after every kind of pose."""
    from top_down_renderer_amd.kernels import DeviceMap, HipKernels
    h, w, res = MAPS[mapname]
    rng = np.random.default_rng(ncls * 7 + h)
    rows, cols = int(F32(h) / F32(res)), int(F32(w) / F32(res))
    k = HipKernels()
    dm = DeviceMap(k.zeros((4,)), ncls, rows, cols, res)
    votes, dirty, counters = k.fuse_state(dm)
    want = np.zeros((ncls, rows, cols), np.uint32)
    tot, want_dirty = [0, 0], set()

    def add(scan, srows, scols, polar, pose, cells):
        a, d = FR.add_votes(want, scan, cells)
        tot[0], tot[1] = tot[0] + a, tot[1] + d
        want_dirty.update(FR.dirty_tiles(scan, cells, cols))
        k.fuse_votes(dm, [k.to_device(scan.reshape(ncls, scols, srows))], [polar], [pose], votes, dirty, counters)
        assert counters.cpu().numpy().tolist() == tot, (srows, scols, pose)
        return a, d

    for nb, nr in POLAR:
        ang = F32(2 * np.pi / nb)
        k.set_polar_table(dm, nb, nr, ang)
        tab = no.polar_table(nb, nr, ang, res)
        assert np.array_equal(tab.T, dm.tab_host)
        thetas = [-0.7, 7.5, 0.0] + _boundary(nb)
        for i, (cx, cy) in enumerate(_poses(rows, cols, res)):
            th = thetas[(i + (3 if nb == 100 else 0)) % len(thetas)]
            scale, sres = [1.0, 1.3, 0.8][i % 3], [1.0, 0.7, 2.5][(i + 1) % 3]
            scan = _scan(rng, ncls, nb * nr)
            a, d = add(scan, nb, nr, True, (cx, cy, th, scale, sres),
                       FR.polar_cells(tab, nb, nr, res, rows, cols, cx, cy, th, scale, sres))
            if cx < 0:
                assert a == 0 and d > 0                      # wholly off the map: no vote, all dropped
    for wr, wc in WINDOWS:
        for i, (cx, cy) in enumerate(_poses(rows, cols, res)):
            th, scale, sres = [-2.2, 0.4, 9.0][i % 3], [1.0, 1.25][i % 2], [1.0, 0.8, 1.7][i % 3]
            add(_scan(rng, ncls, wr * wc), wr, wc, False, (cx, cy, th, scale, sres),
                FR.cart_cells(oracle_mod, wr, wc, res, rows, cols, cx, cy, th, scale, sres))
    # single cells on either side of a tile border and in the last row / column (1 x 1 window: the cell of the centre)
    for yi, xi in ((31, 31), (32, 32), (rows - 1, cols - 1), (rows - 1, 0), (0, cols - 1)):
        cells = FR.cart_cells(oracle_mod, 1, 1, res, rows, cols, xi * res, yi * res, 0.3, 1.0, 1.0)
        assert (cells[0][0], cells[1][0], cells[2][0]) == (yi, xi, True)
        assert add(np.full((ncls, 1), 3, F32), 1, 1, False, (xi * res, yi * res, 0.3, 1.0, 1.0), cells) == (3 * ncls, 0)
    assert np.array_equal(votes.cpu().numpy().view(np.uint32), want)
    assert want[:, 31, 31].all() and want[:, 32, 32].all() and want[:, rows - 1, cols - 1].all() and tot[1] > 0
    bits = dirty.cpu().numpy().view(np.uint32)
    n_tiles = ((rows + 31) // 32) * ((cols + 31) // 32)
    assert {t for t in range(32 * len(bits)) if bits[t >> 5] >> (t & 31) & 1} == want_dirty and 4 <= len(want_dirty) <= n_tiles


def test_contention_wrap_and_non_integer_counts(oracle_mod):
    from top_down_renderer_amd.fuse import MapFuser
    ncls, (h, w, res) = 6, MAPS["96x80r1"]
    rng = np.random.default_rng(5)
    m = _make_map(_image(rng, h, w, ncls), ncls, res)
    nb, nr = 100, 25
    m.sample_pts_polar(nb, nr, F32(2 * np.pi / nb))
    fuser = MapFuser(m, np.arange(ncls, dtype=np.uint8), 1, (1, 2))
    # every count in ring 0: all nb bins of every class hit the centre cell
    scan = np.zeros((ncls, nb * nr), F32)
    scan[:, :nb] = 2.0 ** 20
    assert fuser.add_images(_imgs(scan, nb, nr), True, (40.0, 50.0, 1.0, 1.0), 1.0) == (ncls * nb * 2 ** 20, 0)
    v = fuser.votes()
    assert (v[:, 50, 40] == nb * 2 ** 20).all() and int(v.astype(np.uint64).sum()) == ncls * nb * 2 ** 20
    # a cell driven past 2^32 wraps
    big = np.full((ncls, 1), 2.0 ** 31 - 128, F32)
    for _ in range(3):
        fuser.add_images(big.reshape(ncls, 1, 1), False, (7.0, 9.0, 0.0, 1.0), 1.0)
    assert (fuser.votes()[:, 9, 7] == (3 * (2 ** 31 - 128)) % 2 ** 32).all()
    # NaN / -1 / 0.5 / 2^31 vote 0: nothing added, nothing dropped, no dirty tile
    before = fuser.votes()
    fuser.apply()
    bad = np.tile(np.asarray([np.nan, -1.0, 0.5, 2.0 ** 31, 0.99999994, -np.inf], F32), (ncls, 1))
    assert fuser.add_images(_imgs(bad, 3, 2), False, (20.0, 20.0, 0.0, 1.0), 1.0) == (0, 0)
    assert np.array_equal(fuser.votes(), before) and fuser.apply() == 0


def test_adjoint_identity_on_the_device(oracle_mod):
    """sum V * M == sum S * L: the votes of tdr_fuser_add_images against tdr_map_local_map of the same map and pose, and
    the map's own records: the scatter is the transpose of the gather the project already trusts."""
    from top_down_renderer_amd._lib import check
    from top_down_renderer_amd.fuse import MapFuser
    ncls, (h, w, res) = 6, MAPS["97x81r2"]
    rng = np.random.default_rng(9)
    m = _make_map(_image(rng, h, w, ncls), ncls, res)
    nb, nr = 16, 9
    m.sample_pts_polar(nb, nr, F32(2 * np.pi / nb))
    _, M, _, _ = _records(m)
    for polar, rows, cols, pose, sres in ((True, nb, nr, (70.0, 40.0, 2.3, 1.2), 3.0), (True, nb, nr, (3.0, 90.0, -1.0, 1.0), 4.0),
                                          (False, 7, 5, (60.0, 33.0, 0.9, 1.0), 2.5), (False, 33, 32, (60.0, 80.0, 4.0, 1.2), 1.5)):
        fuser = MapFuser(m, np.arange(ncls, dtype=np.uint8), 1, (1, 2))
        scan = _scan(rng, ncls, rows * cols)
        fuser.add_images(_imgs(scan, rows, cols), polar, pose, sres)
        V = fuser.votes()
        L = np.zeros((ncls, rows * cols), F32)
        k = np.zeros(rows * cols, np.uint8)
        cx, cy, th, scale = pose
        check(m.L.tdr_map_local_map(m.h, int(polar), C.c_float(cx), C.c_float(cy), C.c_float(scale if polar else th),
                                    C.c_float(sres if polar else F32(sres) * F32(scale)), rows, cols, L.ctypes.data_as(vp),
                                    k.ctypes.data_as(vp)))
        if polar:
            b = np.arange(nb * nr)
            L = L[:, (b % nb - no.rot_shift(th, nb)) % nb + nb * (b // nb)]
        lhs = math.fsum((V.astype(np.float64) * M.astype(np.float64)).ravel())
        rhs = math.fsum((scan.astype(np.float64) * L.astype(np.float64)).ravel())
        assert lhs == rhs and lhs > 0, (polar, rows, cols)


# ---- batch -----------------------------------------------------------------------------------------------------------------------
def _renders(rng, m, ncls, k, nb, nr, win):
    from top_down_renderer_amd import batch
    out = []
    for i in range(k):
        r = batch.Renderer(_lut(ncls))
        pts = np.zeros((400, 4), F32)
        pts[:, :3] = rng.normal(0, 6, (400, 3))
        pts[:, 3] = rng.integers(0, ncls + 1, 400)
        if i % 3 == 2:
            r.render_cart(pts, 4, 3, 0.9, ncls, win[0], win[1])
        else:
            r.render_polar(pts, 4, 3, 1.1, F32(2 * np.pi / nb), ncls, nb, nr)
        out.append(r)
    return out


@pytest.mark.parametrize("k", [1, 2, 7])
def test_add_batch_equals_the_single_adds(k, oracle_mod):
    from top_down_renderer_amd.fuse import MapFuser
    ncls, (h, w, res) = 6, MAPS["96x80r1"]
    rng = np.random.default_rng(20 + k)
    m = _make_map(_image(rng, h, w, ncls), ncls, res)
    nb, nr = 16, 9
    m.sample_pts_polar(nb, nr, F32(2 * np.pi / nb))
    rs = _renders(rng, m, ncls, k, nb, nr, (7, 5))
    poses = [(rng.uniform(-5, w + 5), rng.uniform(-5, h + 5), rng.uniform(-4, 8), rng.uniform(0.7, 1.4), rng.uniform(0.6, 2.0))
             for _ in range(k)]
    cl = np.arange(ncls, dtype=np.uint8)
    a, b, c = (MapFuser(m, cl, 1, (1, 2)) for _ in range(3))
    tot = a.add_scans(rs, poses)
    singles = [b.add_scan(r, p[:4], p[4]) for r, p in zip(rs, poses)]
    for r, p in reversed(list(zip(rs, poses))):                  # the other order
        c.add_scan(r, p[:4], p[4])
    assert tot == (sum(s[0] for s in singles), sum(s[1] for s in singles)) and tot[0] > 0
    assert np.array_equal(a.votes(), b.votes()) and np.array_equal(a.votes(), c.votes())
    # ... and the restatement on the renders read back
    want = np.zeros_like(a.votes())
    tab = no.polar_table(nb, nr, F32(2 * np.pi / nb), res)
    for i, (r, p) in enumerate(zip(rs, poses)):
        img, _ = r.get_render()
        scan = np.ascontiguousarray(img.transpose(0, 2, 1)).reshape(ncls, -1)
        if i % 3 == 2:
            cells = FR.cart_cells(oracle_mod, 7, 5, res, h, w, p[0], p[1], p[2], p[3], p[4])
        else:
            cells = FR.polar_cells(tab, nb, nr, res, h, w, p[0], p[1], p[2], p[3], p[4])
        FR.add_votes(want, scan, cells)
    assert np.array_equal(a.votes(), want)


def test_add_reads_a_batched_render_in_order():
    """tdr_batch_render_polar does not wait for its kernels: the adds that follow read the renders behind the renderers'
    events, and the next batched render waits for those reads.  Votes equal the restatement on the renders read back."""
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.fuse import MapFuser
    ncls, (h, w, res) = 6, MAPS["96x80r1"]
    rng = np.random.default_rng(27)
    m = _make_map(_image(rng, h, w, ncls), ncls, res)
    nb, nr = 100, 25
    ang = F32(2 * np.pi / nb)
    m.sample_pts_polar(nb, nr, ang)
    tab = no.polar_table(nb, nr, ang, res)
    rs = [batch.Renderer(_lut(ncls)) for _ in range(3)]
    fuser = MapFuser(m, np.arange(ncls, dtype=np.uint8), 1, (1, 2))
    want = np.zeros((ncls, h, w), np.uint32)
    for rnd in range(2):
        clouds = []
        for _ in rs:
            pts = np.zeros((3000, 4), F32)
            pts[:, :3] = rng.normal(0, 9, (3000, 3))
            pts[:, 3] = rng.integers(0, ncls, 3000)
            clouds.append((pts, 4, 3))
        batch.render_batch(rs, clouds, 1.0, ang, ncls, nb, nr)
        poses = [(rng.uniform(10, w - 10), rng.uniform(10, h - 10), rng.uniform(-3, 3), 1.0, 1.0) for _ in rs]
        if rnd == 0:
            got = fuser.add_scans(rs, poses)
        else:
            singles = [fuser.add_scan(r, p[:4], p[4]) for r, p in zip(rs, poses)]
            got = (sum(x[0] for x in singles), sum(x[1] for x in singles))
        tot = [0, 0]
        for r, p in zip(rs, poses):
            img, _ = r.get_render()
            scan = np.ascontiguousarray(img.transpose(0, 2, 1)).reshape(ncls, -1)
            a, d = FR.add_votes(want, scan, FR.polar_cells(tab, nb, nr, res, h, w, *p))
            tot[0], tot[1] = tot[0] + a, tot[1] + d
        assert got == tuple(tot) and tot[0] > 1000
    assert np.array_equal(fuser.votes(), want)


# ---- labels and apply -------------------------------------------------------------------------------------------------------------
def _particles(poses):
    from top_down_renderer_amd import batch
    st = np.zeros(len(poses), batch.STATE_DTYPE)
    for i, (cx, cy, th) in enumerate(poses):
        st[i]["init_x_px"], st[i]["init_y_px"], st[i]["theta"], st[i]["scale"], st[i]["have_init"] = cx, cy, th, 1.0, 1
    return st


@pytest.mark.parametrize("mapname", list(MAPS))
def test_apply_gives_the_fused_image_and_a_map_equal_to_a_fresh_one(mapname, oracle_mod):
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.fuse import MapFuser
    ncls, (h, w, res) = 6, MAPS[mapname]
    rng = np.random.default_rng(31)
    img = _image(rng, h, w, ncls)
    # raw labels: class c is written as 10 + c; the image holds 10 + c too, except some cells that hold the alias 40 + c
    lut = np.full(256, -1, np.int32)
    lut[10:10 + ncls] = np.arange(ncls)
    lut[40:40 + ncls] = np.arange(ncls)
    img = np.where(img == UNKNOWN, UNKNOWN, img + np.where(rng.random((h, w)) < 0.3, 40, 10)).astype(np.uint8)
    cl = (10 + np.arange(ncls)).astype(np.uint8)
    m = batch.MapHandle.from_labels(img, lut, ncls, res, (3, 4))
    nb, nr = 16, 9
    ang = F32(2 * np.pi / nb)
    m.sample_pts_polar(nb, nr, ang)
    rows, cols = int(F32(h) / F32(res)), int(F32(w) / F32(res))
    poses3 = [(0.4 * cols * res, 0.5 * rows * res, 0.3), (0.7 * cols * res, 0.3 * rows * res, 2.0)]
    f1 = batch.FilterHandle(m, 2, pkg.FilterParams(fixed_scale=1.0), seed=3)
    f2 = batch.FilterHandle(m, 2, pkg.FilterParams(fixed_scale=1.0), seed=4)
    for f in (f1, f2):
        f.configure(1)
        f.set_states(_particles(poses3))
    fuser = MapFuser(m, cl, 3, (1, 2))
    tab = no.polar_table(nb, nr, ang, res)
    votes = np.zeros((ncls, rows, cols), np.uint32)
    for k in range(6):
        cx, cy, th = rng.uniform(0, cols * res), rng.uniform(0, rows * res), rng.uniform(-3, 3)
        scan = _scan(rng, ncls, nb * nr, hi=9)
        FR.add_votes(votes, scan, FR.polar_cells(tab, nb, nr, res, rows, cols, cx, cy, th, 1.0, 2.0))
        fuser.add_images(_imgs(scan, nb, nr), True, (cx, cy, th, 1.0), 2.0)
    want = FR.fuse_labels(votes, img, cl, 3, 1, 2, res)
    assert (want != img).sum() > 20
    changed = fuser.apply([f1])
    assert np.array_equal(fuser.labels(), want)
    assert changed == FR.changed_cells(img, want, lut, ncls, res) and 0 < changed
    assert changed < (want != img).sum()                          # (alias labels: pixels that changed, classes that did not)
    fresh = batch.MapHandle.from_labels(want, lut, ncls, res, (3, 4))
    fresh.sample_pts_polar(nb, nr, ang)
    got_rec, want_rec = _records(m), _records(fresh)
    assert np.array_equal(got_rec[0], want_rec[0]) and got_rec[3] == want_rec[3]
    assert np.array_equal(got_rec[1], want_rec[1]) and np.array_equal(got_rec[2], want_rec[2])
    assert m.center() == (3, 4)
    # the filter given to apply and one that only shares the map score like a filter created on the fresh map
    f3 = batch.FilterHandle(fresh, 2, pkg.FilterParams(fixed_scale=1.0), seed=5)
    f3.configure(1)
    f3.set_states(_particles(poses3))
    scan = _imgs(_scan(rng, ncls, nb * nr), nb, nr)
    ws = []
    for f in (f1, f2, f3):
        f.compute_weights(scan, 2.0)
        ws.append(f.raw_weights(2))
    assert np.array_equal(ws[0], ws[2]) and np.array_equal(ws[1], ws[2]) and np.isfinite(ws[2]).all()
    # nothing added: nothing changes
    assert fuser.apply([f1, f2]) == 0 and np.array_equal(fuser.labels(), want)
    assert np.array_equal(_records(m)[0], want_rec[0])
    assert fuser.stats()["applies"] == 1


def test_decay_reset_rebase(oracle_mod):
    from top_down_renderer_amd._lib import TdrError
    from top_down_renderer_amd.fuse import MapFuser
    ncls, (h, w, res) = 3, MAPS["96x80r1"]
    rng = np.random.default_rng(41)
    img = np.zeros((h, w), np.uint8)                                # all class 0
    m = _make_map(img, ncls, res)
    cl = np.arange(ncls, dtype=np.uint8)
    fuser = MapFuser(m, cl, 2, (1, 2))
    one = np.zeros((ncls, 1, 1), F32)
    one[1] = 3                                                       # 3 votes for class 1 at cell (row 40, col 33)
    fuser.add_images(one, False, (33.0, 40.0, 0.0, 1.0), 1.0)
    assert fuser.apply() == 1
    want = img.copy()
    want[h - 1 - 40, 33] = 1
    assert np.array_equal(fuser.labels(), want)
    fuser.decay(1)                                                   # 3 >> 1 = 1 < min_votes: the verdict falls back to base
    assert fuser.votes()[1, 40, 33] == 1
    assert fuser.apply() == 1 and np.array_equal(fuser.labels(), img)
    fuser.add_images(one, False, (33.0, 40.0, 0.0, 1.0), 1.0)
    assert fuser.apply() == 1 and fuser.votes()[1, 40, 33] == 4
    fuser.reset()
    assert not fuser.votes().any()
    assert fuser.apply() == 1 and np.array_equal(fuser.labels(), img)
    # another image of the same shape: the votes stay and speak again on the new base
    fuser.add_images(one, False, (33.0, 40.0, 0.0, 1.0), 1.0)
    assert fuser.apply() == 1
    other = np.full((h, w), 2, np.uint8)
    _set_labels(m, other, ncls, res)
    assert fuser.rebase() is True and fuser.votes()[1, 40, 33] == 3
    want = other.copy()
    want[h - 1 - 40, 33] = 1
    assert fuser.apply() == 1 and np.array_equal(fuser.labels(), want)
    # another shape: add is refused until the rebase, which clears the votes
    small = np.zeros((50, 70), np.uint8)
    _set_labels(m, small, ncls, res)
    with pytest.raises(TdrError, match="rebase"):
        fuser.add_images(one, False, (33.0, 40.0, 0.0, 1.0), 1.0)
    with pytest.raises(TdrError, match="rebase"):
        fuser.apply()
    assert fuser.rebase() is False
    assert fuser.votes().shape == (ncls, 50, 70) and not fuser.votes().any()
    assert fuser.apply() == 0 and np.array_equal(fuser.labels(), small)
    fuser.add_images(one, False, (33.0, 40.0, 0.0, 1.0), 1.0)
    assert fuser.apply() == 1 and fuser.labels()[50 - 1 - 40, 33] == 1


# ---- the closed loop ----------------------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_device():
    """The scene of tests/test_fuse_ref.py: after apply the raw weight of a particle at each true pose is strictly greater
    than before, and the fused image is the NumPy one."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.fuse import MapFuser
    sc = FR.closed_loop_scene()
    ncls, nb, nr = sc["ncls"], sc["nb"], sc["nr"]
    m = batch.MapHandle.from_labels(sc["base_img"], sc["lut"], ncls, 1.0)
    m.sample_pts_polar(nb, nr, sc["ang_res"])
    fs = []
    for k, pose in enumerate(sc["poses"]):
        f = batch.FilterHandle(m, 1, pkg.FilterParams(fixed_scale=1.0), seed=7 + k)
        f.configure(1)
        f.set_states(_particles([pose]))
        fs.append(f)

    def weights():
        out = []
        for f, scan in zip(fs, sc["scans"]):
            f.compute_weights(_imgs(scan, nb, nr), sc["res"])
            out.append(float(f.raw_weights(1)[0]))
        return out

    before = weights()
    fuser = MapFuser(m, sc["class_label"], sc["min_votes"], sc["share"])
    for (cx, cy, th), scan in zip(sc["poses"], sc["scans"]):
        fuser.add_images(_imgs(scan, nb, nr), True, (cx, cy, th, 1.0), sc["res"])
    votes, fused = FR.closed_loop_fuse(sc)
    assert np.array_equal(fuser.votes(), votes)
    assert fuser.apply(fs) == FR.changed_cells(sc["base_img"], fused, sc["lut"], ncls, 1.0)
    assert np.array_equal(fuser.labels(), fused)
    after = weights()
    for k, (b, a) in enumerate(zip(before, after)):
        assert a > b, (k, b, a)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_votes_labels_and_map_untouched():
    from top_down_renderer_amd import batch
    from top_down_renderer_amd._lib import TdrError
    from top_down_renderer_amd.fuse import MapFuser
    ncls, (h, w, res) = 6, MAPS["96x80r1"]
    rng = np.random.default_rng(51)
    img = _image(rng, h, w, ncls)
    m = _make_map(img, ncls, res)
    cl = np.arange(ncls, dtype=np.uint8)
    for kw in (dict(min_votes=0), dict(share=(1, 0)), dict(share=(3, 2)), dict(share=(1, 2 ** 24 + 1))):
        with pytest.raises(TdrError):
            MapFuser(m, cl, **kw)
    with pytest.raises(TdrError, match="flatten_lut"):
        MapFuser(m, cl[::-1].copy(), 1, (1, 2))
    with pytest.raises(TdrError, match="resolution"):
        MapFuser(_make_map(img, ncls, 0.5), cl, 1, (1, 2))
    dist = batch.MapHandle(np.zeros((ncls, 8, 8), F32), np.zeros((8, 8), np.uint8), 1.0)
    with pytest.raises(TdrError, match="label image"):
        MapFuser(dist, cl, 1, (1, 2))
    nb, nr = 16, 9
    fuser = MapFuser(m, cl, 1, (1, 2))
    good = _scan(rng, ncls, nb * nr)
    with pytest.raises(TdrError, match="table"):                    # no table yet
        fuser.add_images(_imgs(good, nb, nr), True, (40.0, 40.0, 0.0, 1.0), 1.0)
    m.sample_pts_polar(nb, nr, F32(2 * np.pi / nb))
    fuser.add_images(_imgs(good, nb, nr), True, (40.0, 40.0, 0.0, 1.0), 1.0)
    fuser.apply()
    votes, labels, rec = fuser.votes(), fuser.labels(), _records(m)[0]
    r, r2, empty = batch.Renderer(_lut(ncls)), batch.Renderer(_lut(ncls)), batch.Renderer(_lut(ncls))
    pts = np.ones((10, 4), F32)
    r.render_polar(pts, 4, 3, 1.0, F32(2 * np.pi / nb), ncls, nb, nr)
    r2.render_polar(pts, 4, 3, 1.0, F32(2 * np.pi / 20), ncls, 20, nr)          # not the table's shape
    r5 = batch.Renderer(_lut(5))
    r5.render_polar(pts, 4, 3, 1.0, F32(2 * np.pi / nb), 5, nb, nr)              # another class count
    ok = (40.0, 40.0, 0.0, 1.0)
    for call in (lambda: fuser.add_scan(empty, ok, 1.0), lambda: fuser.add_scan(r2, ok, 1.0), lambda: fuser.add_scan(r5, ok, 1.0),
                 lambda: fuser.add_scans([r, r], [ok + (1.0,)] * 2), lambda: fuser.add_scan(r, (np.nan, 40.0, 0.0, 1.0), 1.0),
                 lambda: fuser.add_scan(r, (40.0, 40.0, np.inf, 1.0), 1.0), lambda: fuser.add_scan(r, (40.0, 40.0, 0.0, 0.0), 1.0),
                 lambda: fuser.add_scan(r, ok, 0.0), lambda: fuser.add_scan(r, ok, -1.0),
                 lambda: fuser.add_images(_imgs(good, nb, nr)[:, :, :5], True, ok, 1.0)):
        with pytest.raises(TdrError):
            call()
    other = _make_map(img, ncls, res)
    import top_down_renderer_amd as pkg
    stranger = batch.FilterHandle(other, 1, pkg.FilterParams(fixed_scale=1.0), seed=1)
    with pytest.raises(TdrError, match="another map"):
        fuser.apply([stranger])
    assert np.array_equal(fuser.votes(), votes) and np.array_equal(fuser.labels(), labels)
    assert np.array_equal(_records(m)[0], rec) and fuser.apply() == 0
    assert fuser.add_scan(r, ok, 1.0)[0] > 0                       # and the fuser still works


# ---- launchers == handle == Python class ---------------------------------------------------------------------------------------------
def test_launchers_equal_the_handle(oracle_mod):
    import torch
    from top_down_renderer_amd.fuse import MapFuser
    from top_down_renderer_amd.kernels import DeviceMap, HipKernels
    ncls, (h, w, res) = 6, MAPS["96x80r1"]
    rng = np.random.default_rng(61)
    img = _image(rng, h, w, ncls)
    k = HipKernels()
    dm = DeviceMap(k.zeros((4,)), ncls, h, w, res)
    nb, nr = 16, 9
    ang = F32(2 * np.pi / nb)
    k.set_polar_table(dm, nb, nr, ang)
    m = _make_map(img, ncls, res)
    m.sample_pts_polar(nb, nr, ang)
    cl = np.arange(ncls, dtype=np.uint8)
    fuser = MapFuser(m, cl, 2, (1, 2))
    votes, dirty, counters = k.fuse_state(dm)
    scans = [_scan(rng, ncls, nb * nr), _scan(rng, ncls, 7 * 5), _scan(rng, ncls, nb * nr)]
    shapes = [(nb, nr), (7, 5), (nb, nr)]
    polar = [True, False, True]
    poses = [(40.0, 50.0, 0.4, 1.0, 1.5), (70.0, 90.0, 1.0, 1.2, 2.0), (-300.0, 50.0, 0.0, 1.0, 1.0)]
    dev = [k.to_device(s.reshape(ncls, c, r)) for s, (r, c) in zip(scans, shapes)]
    k.fuse_votes(dm, dev[:1], polar[:1], poses[:1], votes, dirty, counters)         # the one-scan launcher
    k.fuse_votes(dm, dev[1:], polar[1:], poses[1:], votes, dirty, counters)         # the jobs launcher
    k.synchronize()
    tot = [0, 0]
    want_dirty = set()
    tab = no.polar_table(nb, nr, ang, res)
    for s, (r, c), pl, p in zip(scans, shapes, polar, poses):
        a, d = fuser.add_images(_imgs(s, r, c), pl, p[:4], p[4])
        tot[0], tot[1] = tot[0] + a, tot[1] + d
        cells = (FR.polar_cells(tab, nb, nr, res, h, w, *p) if pl else FR.cart_cells(oracle_mod, r, c, res, h, w, *p))
        want_dirty |= set(FR.dirty_tiles(s, cells, w))
    got = votes.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, fuser.votes()) and counters.cpu().numpy().tolist() == tot and tot[1] > 0
    bits = dirty.cpu().numpy().view(np.uint32)
    assert {t for t in range(9) if bits[t >> 5] >> (t & 31) & 1} == want_dirty and len(want_dirty) >= 2
    # the label pass over the dirty tiles: the image, the count and the rectangle
    base = k.to_device(img)
    current = base.clone()
    tiles = k.to_device(np.asarray(sorted(want_dirty), np.int32))
    n, y0, x0, y1, x1 = k.fuse_labels(votes, img.shape, res, cl, 2, (1, 2), base, current, tiles)
    want = FR.fuse_labels(fuser.votes(), img, cl, 2, 1, 2, res)
    ys, xs = np.nonzero(want != img)
    assert np.array_equal(current.cpu().numpy(), want)
    assert (n, y0, x0, y1, x1) == (len(ys), ys.min(), xs.min(), ys.max(), xs.max()) and n > 0
    fuser.apply()
    assert np.array_equal(fuser.labels(), want)
    assert torch.equal(base, k.to_device(img))


# ---- the C++ class ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def facade_fuse_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_fuse")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_fuse.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip",
                    f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def test_cpp_map_fuser(facade_fuse_exe):
    """MapFuser of include/top_down_render/map_fuser.h on the closed-loop scene: the program adds scan 0 from host images
    and the others through ScanRendererPolar renders in one addScans, applies, and writes renders, votes and labels back:
    the restatement's on those renders."""
    sc = FR.closed_loop_scene()
    ncls, nb, nr, size = sc["ncls"], sc["nb"], sc["nr"], sc["size"]
    d = tempfile.mkdtemp(prefix="tdr_fuse_")
    open(os.path.join(d, "meta.txt"), "w").write(
        f"{ncls} {size} {size} {nb} {nr} {sc['res']} {sc['min_votes']} {sc['share'][0]} {sc['share'][1]} {len(sc['poses'])}\n")
    sc["base_img"].tofile(os.path.join(d, "labels.bin"))
    sc["lut"].astype(np.int32).tofile(os.path.join(d, "lut.bin"))
    np.asarray(sc["poses"], F32).tofile(os.path.join(d, "poses.bin"))
    sc["scans"][0].astype(F32).tofile(os.path.join(d, "scan_0.bin"))
    for k, pts in enumerate(sc["pts"]):
        pts.astype(F32).tofile(os.path.join(d, f"pts_{k}.bin"))
    out = subprocess.run([facade_fuse_exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    scans = [np.fromfile(os.path.join(d, f"out_scan_{k}.bin"), F32).reshape(ncls, nb * nr) for k in range(len(sc["poses"]))]
    assert all(s.sum() > 100 for s in scans)
    votes, fused = FR.closed_loop_fuse(sc, scans)
    assert out.stdout.split() == ["ok", str(FR.changed_cells(sc["base_img"], fused, sc["lut"], ncls, 1.0))], out.stdout
    assert np.array_equal(np.fromfile(os.path.join(d, "out_votes.bin"), np.uint32).reshape(votes.shape), votes)
    assert np.array_equal(np.fromfile(os.path.join(d, "out_labels.bin"), np.uint8).reshape(fused.shape), fused)
