"""Incremental aerial-map updates (csrc/tdr_map_incr.hip, tdr_map_update_labels_incremental / tdr_map_patch_labels).
CPU: argument refusals and the locality claim the update rests on, checked with the oracle's ingest.  GPU: after every
kind of edit the map equals a map built fresh by tdr_map_set_labels from the same image, buffer for buffer, and filters
stepped on both stay bit-identical."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "top_down_renderer_amd")
sys.path.insert(0, ROOT)

from oracle import np_oracle as no   # noqa: E402
from top_down_renderer_amd import _lib, synth   # noqa: E402
from top_down_renderer_amd._lib import MapDescC, check   # noqa: E402

vp = C.c_void_p
TILE = 32


def _img(rng, h, w, ncls, unknown_id=200):
    lab = synth.make_label_image(max(h, w), ncls, rng)[:h, :w]
    return np.where(lab >= 0, lab, unknown_id).astype(np.uint8)[::-1].copy()


def _lut(ncls):
    lut = np.full(256, -1, np.int32)
    lut[:ncls] = np.arange(ncls)
    return lut


def _cells(img, res):
    """the label each map cell samples (the oracle's sampling, src/top_down_map.cpp:137-138)"""
    f32 = np.float32
    img_h, img_w = img.shape
    rows, cols = int(f32(img_h) / f32(res)), int(f32(img_w) / f32(res))
    iy = np.maximum((f32(img_h) - np.arange(rows).astype(f32) * f32(res) - f32(1)).astype(f32).astype(np.int64), 0)
    ix = np.minimum((np.arange(cols).astype(f32) * f32(res)).astype(f32).astype(np.int64), img_w - 1)
    return img[iy[:, None], ix[None, :]]


def _class_words(img, lut, ncls, res):
    lab = _cells(img, res).astype(np.int64)
    c = lut[lab]
    return np.where((c >= 0) & (c < ncls), c, -1)


def _dilate(mask, r):
    """Chebyshev dilation by r cells (a (2r+1)^2 box)"""
    out = mask.copy()
    ys, xs = np.nonzero(mask)
    for y, x in zip(ys, xs):
        out[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_refusals_need_no_device():
    L = _lib.load()
    ch = C.c_int64(7)
    img = np.zeros((8, 8), np.uint8)
    lut = _lut(3)
    assert L.tdr_map_update_labels_incremental(None, img.ctypes.data_as(vp), 8, 8, lut.ctypes.data_as(vp), 256, 3,
                                               C.c_float(1.0), 0, 0, C.byref(ch)) == -1
    assert "null pointer" in L.tdr_last_error().decode()
    assert L.tdr_map_patch_labels(None, img.ctypes.data_as(vp), 0, 0, 8, 8, 0, 0, C.byref(ch)) == -1
    assert L.tdr_map_get_desc(None, None) == -1
    assert L.tdr_filter_update_map_labels_incremental(None, img.ctypes.data_as(vp), 8, 8, lut.ctypes.data_as(vp), 256, 3,
                                                      C.c_float(1.0), 0, 0, C.byref(ch)) == -1
    assert L.tdr_filter_patch_map_labels(None, img.ctypes.data_as(vp), 0, 0, 8, 8, 0, 0, C.byref(ch)) == -1
    d = MapDescC()
    n, c, k = C.c_int(0), C.c_int64(0), C.c_int(0)
    assert L.tdr_k_map_update_labels(None, 8, 8, None, 256, C.byref(d), None, None, -1, None, None, C.byref(n), C.byref(c),
                                     C.byref(k), None) == -1
    assert L.tdr_k_map_dict_counts(C.byref(d), None, None) == -1
    assert L.tdr_k_map_gather_tiles(None, 3, 10, 10, None, 1, None, None, None) == -1
    assert L.tdr_map_incr_tiles(4000, 4000) == 125 * 125 and L.tdr_map_incr_tiles(33, 1) == 2
    assert L.tdr_map_incr_tiles(0, 5) == 0
    assert L.tdr_map_incr_workspace_bytes(4000, 4000) >= 125 * 125 * 13


@pytest.mark.parametrize("res", [0.5, 1.0, 2.0])
def test_locality_of_the_distance_maps(res):
    """A cell whose class did not change and that has no changed cell within R = ceil(50 / res) keeps its distances
    bit for bit: the fact the incremental update rests on."""
    ncls = 4
    lut = _lut(ncls)
    R = int(np.ceil(50.0 / res))
    for seed in range(3):
        rng = np.random.default_rng(seed + int(res * 10))
        h, w = (160, 190) if res >= 1 else (90, 110)
        a = _img(rng, h, w, ncls)
        b = a.copy()
        changed = np.zeros(1, bool)
        while not changed.any():                                 # (an edit no cell samples changes nothing)
            for _ in range(1 + seed):
                y, x = rng.integers(0, h - 12), rng.integers(0, w - 12)
                b[y:y + rng.integers(1, 12), x:x + rng.integers(1, 12)] = rng.integers(0, ncls + 1)
            if seed == 2:
                b[rng.integers(0, h), rng.integers(0, w)] = 200  # a cell made unknown
            changed = _class_words(a, lut, ncls, res) != _class_words(b, lut, ncls, res)
        ma, ka = no.load_compressed_raster_map(a, lut, ncls, res)
        mb, kb = no.load_compressed_raster_map(b, lut, ncls, res)
        outside = ~_dilate(changed, R)
        assert np.array_equal(ma[:, outside], mb[:, outside]) and np.array_equal(ka[outside], kb[outside])
        # ... and the claim is not empty: distances differ somewhere inside the dilated set
        assert not np.array_equal(ma, mb) or not np.array_equal(ka, kb)


# ---- GPU helpers --------------------------------------------------------------------------------------------------------
_hip = None


def _read(ptr, nbytes):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    out = np.zeros(nbytes, np.uint8)
    if nbytes:
        assert _hip.hipDeviceSynchronize() == 0
        assert _hip.hipMemcpy(out.ctypes.data_as(vp), vp(ptr), C.c_size_t(nbytes), 2) == 0
    return out


class Map:
    def __init__(self):
        self.L = _lib.load()
        self.h = vp()
        check(self.L.tdr_map_create(C.byref(self.h)))

    def set_labels(self, img, lut, ncls, res, center=(0, 0)):
        check(self.L.tdr_map_set_labels(self.h, img.ctypes.data_as(vp), img.shape[0], img.shape[1], lut.ctypes.data_as(vp),
                                        len(lut), ncls, C.c_float(res), int(center[0]), int(center[1])))

    def incremental(self, img, lut, ncls, res, center=(0, 0)):
        ch = C.c_int64(-2)
        check(self.L.tdr_map_update_labels_incremental(self.h, img.ctypes.data_as(vp), img.shape[0], img.shape[1],
                                                       lut.ctypes.data_as(vp), len(lut), ncls, C.c_float(res),
                                                       int(center[0]), int(center[1]), C.byref(ch)))
        return ch.value

    def patch(self, patch, y0, x0, center=(0, 0)):
        patch = np.ascontiguousarray(patch, np.uint8)
        ch = C.c_int64(-2)
        check(self.L.tdr_map_patch_labels(self.h, patch.ctypes.data_as(vp), y0, x0, patch.shape[0], patch.shape[1],
                                          int(center[0]), int(center[1]), C.byref(ch)))
        return ch.value

    def desc(self):
        d = MapDescC()
        check(self.L.tdr_map_get_desc(self.h, C.byref(d)))
        return d

    def info(self):
        n, r, c, hm = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        res = C.c_float()
        check(self.L.tdr_map_info(self.h, C.byref(n), C.byref(r), C.byref(c), C.byref(res), C.byref(hm)))
        cx, cy = C.c_int(), C.c_int()
        check(self.L.tdr_map_center(self.h, C.byref(cx), C.byref(cy)))
        return n.value, r.value, c.value, res.value, hm.value, cx.value, cy.value

    def buffers(self):
        """every byte the descriptor's buffers define"""
        L, d = self.L, self.desc()
        ncls, rows, cols = d.ncls, d.rows, d.cols
        out = {"rec": _read(d.rec, 4 * int(L.tdr_map_rec_floats_total(ncls, rows, cols))),
               "scalars": (d.ncls, d.rows, d.cols, d.rec_floats, d.resolution, d.cwords, d.dict_n, bool(d.crec),
                           bool(d.dict))}
        if d.cwords:
            out["dict"] = _read(d.dict, 4 * 4096)
            if d.dict_n > 1024:   # the wide form
                out["crec"] = _read(d.crec, 4 * int(L.tdr_cmap_wide_words_total(ncls, rows, cols)))
            else:                 # tiles + known mask; class planes; coarse mask (the padding between is never written)
                tiles = int(L.tdr_cmap_tile_words(ncls, rows, cols))
                kwords = ((rows >> 5) + 2) * ((cols >> 5) + 2) * 32
                out["crec"] = _read(d.crec, 4 * (tiles + kwords))
                pw = int(L.tdr_cmap_plane_words(ncls, rows, cols))
                if pw:
                    off = int(L.tdr_cmap_plane_offset_words(ncls, rows, cols))
                    cm = int(L.tdr_cmap_cmask_words(ncls, rows, cols))
                    out["planes"] = _read(d.crec + 4 * off, 4 * (pw * ncls + cm))
        return out

    def classes(self):
        n, rows, cols, res, hm, _, _ = self.info()
        if not hm:
            return None
        out = np.zeros((rows, cols), np.uint32)
        b = C.c_uint32()
        for y in range(rows):
            for x in range(cols):
                check(self.L.tdr_map_classes_at_point(self.h, int(x * res), int(y * res), C.byref(b)))
                out[y, x] = b.value
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.L.tdr_map_destroy(self.h)
            self.h = None


def _same(a, b, with_classes=True):
    ba, bb = a.buffers(), b.buffers()
    assert ba.keys() == bb.keys()
    for key in ba:
        if key == "scalars":
            assert ba[key] == bb[key]
        else:
            assert np.array_equal(ba[key], bb[key]), key
    assert a.info() == b.info()
    if with_classes:
        ca, cb = a.classes(), b.classes()
        assert (ca is None) == (cb is None)
        if ca is not None:
            assert np.array_equal(ca, cb)


def _fresh(img, lut, ncls, res, center):
    m = Map()
    m.set_labels(img, lut, ncls, res, center)
    return m


def _nchanged(a, b, lut, ncls, res):
    return int((_class_words(a, lut, ncls, res) != _class_words(b, lut, ncls, res)).sum())


def _expected(a, b, lut, ncls, res):
    """what tdr_map_update_labels_incremental reports: the changed-cell count, or -1 when the changed tiles dilated by
    ceil(R / 32) tiles hold more than half the map (TDR_MAP_INCR_MAX_FRACTION)"""
    ch = _class_words(a, lut, ncls, res) != _class_words(b, lut, ncls, res)
    rows, cols = ch.shape
    ty, tx = -(-rows // TILE), -(-cols // TILE)
    t = np.zeros((ty * TILE, tx * TILE), bool)
    t[:rows, :cols] = ch
    t = t.reshape(ty, TILE, tx, TILE).any(axis=(1, 3))
    D = -(-int(np.ceil(50.0 / res)) // TILE)
    aff = _dilate(t, D).sum() if t.any() else 0
    return -1 if aff * TILE * TILE > int(rows * cols * 0.5) else int(ch.sum())


# ---- GPU: edit cases ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("res,ncls", [(1.0, 6), (0.5, 4), (2.0, 3), (1.0, 13)])
def test_edits_match_a_fresh_build(res, ncls):
    rng = np.random.default_rng(int(res * 100) + ncls)
    h, w = {1.0: (600, 560), 0.5: (300, 300), 2.0: (600, 560)}[res]
    lut = _lut(ncls)
    img = _img(rng, h, w, ncls)
    m = Map()
    assert m.incremental(img, lut, ncls, res, (3, 4)) == -1          # no previous map: the full path
    _same(m, _fresh(img, lut, ncls, res, (3, 4)))

    def step(new, center, expect_changed=True):
        nonlocal img
        got = m.incremental(new, lut, ncls, res, center)
        assert got == _expected(img, new, lut, ncls, res)
        if expect_changed:
            assert got != 0
        img = new
        _same(m, _fresh(img, lut, ncls, res, center), with_classes=ncls < 13)

    py, px = h - 1 - 2 * (h // 4), 2 * (w // 6)                                                # sampled at every res
    b = img.copy(); b[py, px] = (b[py, px] + 1) % ncls                                        # one pixel
    step(b, (3, 4))
    b = img.copy(); b[40:90, 60:140] = 1                                                      # one rectangle
    step(b, (5, 4))
    b = img.copy()                                                                            # scattered over many tiles
    for _ in range(6):
        y, x = rng.integers(0, h), rng.integers(0, w)
        b[y, x] = rng.integers(0, ncls)
    step(b, (5, 4))
    b = img.copy(); b[0:3, :] = 0; b[:, -2:] = 2 % ncls; b[-1, 0] = 1; b[h - 5:, w - 5:] = 0  # border and corners
    step(b, (5, 4))
    b = img.copy(); b[100:130, 20:60] = 200; b[h - 7, 7] = 255                                    # cells made unknown
    step(b, (5, 4))
    step(img.copy(), (17, -9), expect_changed=False)                                          # no change, moved centre
    # a changed shape, resolution or LUT: the full path
    b = img[:-20].copy()
    assert m.incremental(b, lut, ncls, res, (1, 1)) == -1
    _same(m, _fresh(b, lut, ncls, res, (1, 1)), with_classes=False)
    lut2 = lut.copy(); lut2[0], lut2[1] = 1, 0
    assert m.incremental(b, lut2, ncls, res, (1, 1)) == -1
    _same(m, _fresh(b, lut2, ncls, res, (1, 1)), with_classes=False)
    assert m.incremental(b, lut2, ncls, res * 2, (1, 1)) == -1
    _same(m, _fresh(b, lut2, ncls, res * 2, (1, 1)), with_classes=False)


@pytest.mark.gpu
def test_dictionary_changes_take_the_compaction_fallback():
    ncls, res = 4, 1.0
    lut = _lut(ncls)
    rng = np.random.default_rng(5)
    img = _img(rng, 400, 460, ncls)
    img[img == 3] = 0
    img[20:24, 30:33] = 3                              # class 3: one small blob
    m = Map()
    m.set_labels(img, lut, ncls, res)
    n0 = m.desc().dict_n
    b = img.copy(); b[20:24, 30:33] = 0                # the last cells of class 3 go: its distances become 50 everywhere
    assert m.incremental(b, lut, ncls, res) == 12 == _expected(img, b, lut, ncls, res)
    assert m.desc().dict_n != n0                       # the dictionary changed: only a full compaction gets it right
    _same(m, _fresh(b, lut, ncls, res, (0, 0)))
    # distance values the dictionary lacks: every 2 x 2 block holds all four classes (distances 0, 1, sqrt(2)), then a
    # 40 x 40 block of class 0 puts the other classes up to 20 cells away
    yy, xx = np.mgrid[0:400, 0:400]
    img = ((yy % 2) * 2 + (xx % 2)).astype(np.uint8)
    m2 = Map()
    m2.set_labels(img, lut, ncls, res)
    n0 = m2.desc().dict_n
    b = img.copy(); b[200:240, 100:140] = 0
    assert m2.incremental(b, lut, ncls, res) == _expected(img, b, lut, ncls, res) == 1200
    assert m2.desc().dict_n > n0
    _same(m2, _fresh(b, lut, ncls, res, (0, 0)))
    # the counts are rebuilt after the fallback: further edits stay exact
    c = b.copy(); c[300:310, 300:310] = 3
    assert m2.incremental(c, lut, ncls, res) == _expected(b, c, lut, ncls, res) == 75
    _same(m2, _fresh(c, lut, ncls, res, (0, 0)))


@pytest.mark.gpu
def test_patch_and_random_sequence():
    ncls, res = 6, 1.0
    lut = _lut(ncls)
    rng = np.random.default_rng(11)
    img = _img(rng, 520, 600, ncls)
    m = Map()
    with pytest.raises(_lib.TdrError):
        m.patch(np.zeros((2, 2), np.uint8), 0, 0)     # no previous label-image map
    m.set_labels(img, lut, ncls, res, (1, 2))
    with pytest.raises(_lib.TdrError):
        m.patch(np.zeros((2, 2), np.uint8), 519, 0)   # outside the image
    p = rng.integers(0, ncls + 1, (17, 23)).astype(np.uint8)
    new = img.copy(); new[100:117, 200:223] = p
    assert m.patch(p, 100, 200, (4, 4)) == _nchanged(img, new, lut, ncls, res)
    img = new
    _same(m, _fresh(img, lut, ncls, res, (4, 4)))
    for i in range(20):                               # 20 random updates in a row, full images and patches
        b = img.copy()
        for _ in range(rng.integers(1, 4)):
            y, x = rng.integers(0, 500), rng.integers(0, 580)
            b[y:y + rng.integers(1, 40), x:x + rng.integers(1, 60)] = rng.integers(0, ncls + 1)
        want = _nchanged(img, b, lut, ncls, res)
        if i % 3 == 2:
            y, x = rng.integers(0, 460), rng.integers(0, 530)
            b = img.copy(); b[y:y + 50, x:x + 60] = rng.integers(0, ncls, (50, 60))
            want = _nchanged(img, b, lut, ncls, res)
            got = m.patch(b[y:y + 50, x:x + 60], y, x, (i, -i))
        else:
            got = m.incremental(b, lut, ncls, res, (i, -i))
            want = _expected(img, b, lut, ncls, res)
        assert got == want
        img = b
        _same(m, _fresh(img, lut, ncls, res, (i, -i)), with_classes=(i % 5 == 0))


@pytest.mark.gpu
def test_static_map_then_incremental_takes_the_full_path(tmp_path):
    ncls, res = 3, 1.0
    lut = _lut(ncls)
    rng = np.random.default_rng(2)
    img = _img(rng, 400, 420, ncls)
    a = Map()
    a.set_labels(img, lut, ncls, res)
    d = str(tmp_path / "rasters").encode()
    check(a.L.tdr_map_save_rasters(a.h, d))
    m = Map()
    check(m.L.tdr_map_load_rasters(m.h, d, ncls, C.c_float(res), 0, 0))   # a static map (the raster cache)
    b = img.copy(); b[5:9, 5:9] = 1
    assert m.incremental(b, lut, ncls, res, (2, 2)) == -1
    _same(m, _fresh(b, lut, ncls, res, (2, 2)))
    c = b.copy(); c[50, 50] = (b[50, 50] + 1) % ncls
    assert m.incremental(c, lut, ncls, res, (2, 2)) == _expected(b, c, lut, ncls, res) == 1
    _same(m, _fresh(c, lut, ncls, res, (2, 2)))


@pytest.mark.gpu
def test_large_map_edit():
    ncls, res = 6, 1.0
    lut = _lut(ncls)
    rng = np.random.default_rng(4000)
    lab = synth.make_label_image(4000, ncls, rng)
    img = np.where(lab >= 0, lab, 200).astype(np.uint8)[::-1].copy()
    m = Map()
    m.set_labels(img, lut, ncls, res)
    b = img.copy(); b[1000:1064, 2000:2064] = 2; b[3990:, :12] = 1
    assert m.incremental(b, lut, ncls, res, (9, 9)) == _nchanged(img, b, lut, ncls, res) > 0
    _same(m, _fresh(b, lut, ncls, res, (9, 9)), with_classes=False)


# ---- GPU: filters on the two maps ------------------------------------------------------------------------------------
class _Empty:
    def __init__(self, m, ncls):
        self.h, self.ncls = m.h, ncls


@pytest.mark.gpu
def test_filters_on_incremental_and_fresh_maps_step_identically():
    from top_down_renderer_amd import batch
    from top_down_renderer_amd.particle_filter import FilterParams
    ncls, res, nb, nr, ang_res = 4, 1.0, 64, 32, float(2 * np.pi / 64)
    lut = _lut(ncls)
    rng = np.random.default_rng(21)
    img0 = _img(rng, 480, 520, ncls)
    img1 = img0.copy(); img1[60:100, 80:150] = 1; img1[200:210, 10:20] = 200
    ma, mb = Map(), Map()
    for m in (ma, mb):
        check(m.L.tdr_map_sample_pts_polar(m.h, nb, nr, C.c_float(ang_res)))
    fa = batch.FilterHandle(_Empty(ma, ncls), 3000, FilterParams().to_c(ncls), seed=9)
    fb = batch.FilterHandle(_Empty(mb, ncls), 3000, FilterParams().to_c(ncls), seed=9)
    L = ma.L
    ch = C.c_int64(0)

    def full(f, img, center):
        check(L.tdr_filter_update_map_labels(f.h, img.ctypes.data_as(vp), img.shape[0], img.shape[1],
                                             lut.ctypes.data_as(vp), len(lut), ncls, C.c_float(res), *center))

    def incr(f, img, center):
        check(L.tdr_filter_update_map_labels_incremental(f.h, img.ctypes.data_as(vp), img.shape[0], img.shape[1],
                                                         lut.ctypes.data_as(vp), len(lut), ncls, C.c_float(res),
                                                         *center, C.byref(ch)))
        return ch.value

    full(fa, img0, (120, 130))
    assert incr(fb, img0, (120, 130)) == -1            # the first map: full path, particles initialised
    full(fa, img1, (118, 133))
    assert incr(fb, img1, (118, 133)) == _expected(img0, img1, lut, ncls, res) > 0
    assert np.array_equal(fa.states(), fb.states()) and fa.num_particles() > 0
    _same(ma, mb, with_classes=False)
    # a second filter on map B: its update finds nothing changed and only shifts its particles
    fb2 = batch.FilterHandle(_Empty(mb, ncls), 3000, FilterParams().to_c(ncls), seed=9)
    assert incr(fb2, img1, (118, 133)) == 0
    pts = np.zeros((4000, 4), np.float32)
    r = rng.uniform(2, 30, 4000); t = rng.uniform(0, 2 * np.pi, 4000)
    pts[:, 0], pts[:, 1], pts[:, 3] = r * np.cos(t), r * np.sin(t), rng.integers(0, ncls, 4000)
    ren = batch.Renderer(lut)
    ren.render_polar(pts, 4, 3, 1.0, ang_res, ncls, nb, nr)
    for step in range(2):                              # the first update runs the 40-rotation search
        for f in (fa, fb):
            f.propagate(0.5, 0.1, 0.02)
            f.update(ren, 1.0)
        n = fa.num_particles()
        assert n == fb.num_particles()
        assert np.array_equal(fa.states(), fb.states()), step
        ra, rb = fa.raw_weights(n), fb.raw_weights(n)
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), (step, int((ra.view(np.uint32) != rb.view(np.uint32)).sum()))
        assert np.array_equal(fa.weights().view(np.uint32), fb.weights().view(np.uint32)), step
        assert np.array_equal(fa.resample_indices(), fb.resample_indices()), step


# ---- GPU: the Python classes ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_update_map_incremental_equals_load():
    import torch
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd.kernels import HipKernels
    k = HipKernels()
    ncls, res = 5, 1.0
    lut = _lut(ncls)
    rng = np.random.default_rng(8)
    img = _img(rng, 400, 380, ncls)
    params = dict(resolution=res, num_classes=ncls, flatten_lut=list(lut))
    m = pkg.TopDownMapPolar(pkg.Params(**params), kernels=k)
    assert m.updateMapIncremental(img, (2, 3)) == -1
    for i in range(6):
        b = img.copy()
        y, x = rng.integers(0, 370), rng.integers(0, 350)
        b[y:y + rng.integers(1, 30), x:x + rng.integers(1, 30)] = rng.integers(0, ncls + 1)
        if i == 3:
            b[b == 4] = 0                              # a class disappears: the dictionary changes
        got = m.updateMapIncremental(b, (2 + i, 3))
        assert got == _expected(img, b, lut, ncls, res)
        img = b
        ref = pkg.TopDownMapPolar(pkg.Params(**params), kernels=k)
        ref.loadCompressedRasterMap(img, (2 + i, 3))
        assert torch.equal(m.dev.rec, ref.dev.rec)
        assert (m.dev.desc.cwords, m.dev.desc.dict_n) == (ref.dev.desc.cwords, ref.dev.desc.dict_n)
        if ref.dev.desc.cwords:
            assert torch.equal(m.dev.dict, ref.dev.dict)
            L = k.lib
            tiles = int(L.tdr_cmap_tile_words(ncls, m.dev.rows, m.dev.cols)) + ((m.dev.rows >> 5) + 2) * ((m.dev.cols >> 5) + 2) * 32
            assert torch.equal(m.dev.crec[:tiles], ref.dev.crec[:tiles])
            pw = int(L.tdr_cmap_plane_words(ncls, m.dev.rows, m.dev.cols))
            if pw:
                off = int(L.tdr_cmap_plane_offset_words(ncls, m.dev.rows, m.dev.cols))
                assert torch.equal(m.dev.crec[off:], ref.dev.crec[off:])
        assert np.array_equal(m.maps_cm_host, ref.maps_cm_host)
        assert m.haveMap() == ref.haveMap() and m.mapCenter() == ref.mapCenter()


# ---- C++: two cores, aerialMap against aerialMapIncremental ------------------------------------------------------------------
@pytest.fixture(scope="module")
def incr_exe():
    from top_down_renderer_amd import build
    build.build()
    exe = os.path.join(tempfile.mkdtemp(prefix="tdr_facade_"), "facade_map_incremental")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_map_incremental.cpp"), "-o", exe, "-L", PKG, "-ltdr_hip",
                    f"-Wl,-rpath,{PKG}"], check=True)
    return exe


def test_facade_map_incremental_compiles(incr_exe):
    assert os.access(incr_exe, os.X_OK)


@pytest.mark.gpu
def test_core_aerial_map_incremental_matches_aerial_map(incr_exe):
    ncls, h, w, steps = 4, 420, 440, 6
    rng = np.random.default_rng(31)
    d = tempfile.mkdtemp(prefix="tdr_map_incr_")
    img = _img(rng, h, w, ncls)
    imgs = [img]
    for _ in range(steps - 1):
        b = imgs[-1].copy()
        y, x = rng.integers(0, h - 30), rng.integers(0, w - 30)
        b[y:y + 30, x:x + 30] = rng.integers(0, ncls + 1)
        imgs.append(b)
    np.stack(imgs).tofile(os.path.join(d, "imgs.bin"))
    pts = np.zeros((3000, 4), np.float32)
    r = rng.uniform(2, 30, 3000); t = rng.uniform(0, 2 * np.pi, 3000)
    pts[:, 0], pts[:, 1], pts[:, 3] = r * np.cos(t), r * np.sin(t), rng.integers(0, ncls, 3000)
    pts.tofile(os.path.join(d, "pts.bin"))
    open(os.path.join(d, "meta.txt"), "w").write(f"{ncls} {h} {w} {steps}\n")
    out = subprocess.run([incr_exe, d], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "ok", out.stdout
    changed = [int(l.split()[2]) for l in lines[:-1]]
    assert changed[0] == -1 and all(c >= 0 for c in changed[1:]) and any(c > 0 for c in changed[1:])
