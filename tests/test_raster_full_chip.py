"""The keyed scan raster cut into a tile per CU, its keys read as 16-byte vectors (csrc/tdr_raster_dev.h:
raster_shape, raster_tile_count_keys), standalone and batched: every image is the CPU oracle's, count for count, and the
packed records are those counts again (NumPy).  Counts are integers, so `array_equal` is the tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCLS = 6
# rows x cols.  16 x 515: the only shape here whose keyed tile keeps two columns (515 = 257 tiles of 2 + 1 of 1); the others
# are a column per tile with a key workspace, and (100 x 25, 256 x 256 without one) tiles that do not divide the columns
SHAPES = [(16, 8), (100, 25), (256, 256), (16, 515)]
# vector tail: no vector at all, 3 tail keys, none, 1; 4099: one round of the vector loop, only its first load in range, + 3
# tail keys; 20 483 (> 4 vectors x 1024 threads x 4 keys): all four loads in flight, a second, partial round, + 3 tail keys
COUNTS = [0, 3, 4, 5, 4099, 20483]


@pytest.fixture(scope="module")
def k():
    import torch
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels()


def _lut():
    lut = np.full(256, -1, np.int32)
    lut[: NCLS + 1] = np.arange(NCLS + 1) - 1   # label 0: no class; labels 1..NCLS: classes 0..NCLS-1
    return lut


def _cloud(rng, n, spread):
    """n points (x, y, z, label): most inside an image of half-width `spread`, some beyond it, some that no image holds
    (NaN / inf coordinates, the origin, labels outside the LUT or without a class)."""
    pts = np.zeros((n, 4), np.float32)
    if n == 0:
        return pts
    pts[:, :2] = rng.normal(0, spread / 2, (n, 2))
    pts[:, 2] = rng.normal(0, 1, n)
    pts[:, 3] = rng.integers(-2, NCLS + 3, n)
    if n > 10:
        m = max(1, n // 50)
        pts[rng.integers(0, n, m), 0] = np.nan
        pts[rng.integers(0, n, m), 1] = np.inf
        pts[rng.integers(0, n, m), 3] = np.nan
        o = rng.integers(0, n, m)
        pts[o, 0] = pts[o, 1] = 0.0
        pts[rng.integers(0, n, m), 3] = 300.0
    return pts


def _records(k, img, rows, cols):
    """The packed records of an image (ncls, rows * cols): record t = row + rows * col holds the class counts, zeros, the
    constant 1 of a spare slot and the total (include/tdr.h: tdr_k_pack_scan)."""
    rf = int(k.lib.tdr_rec_floats(NCLS))
    pk = np.zeros((rows * cols, rf), np.float32)
    pk[:, :NCLS] = img.T
    if NCLS + 2 <= rf:
        pk[:, rf - 2] = 1.0
    pk[:, rf - 1] = img.sum(axis=0)
    return pk.reshape(-1)


def _oracle(oracle, polar, pts, res, ang, rows, cols):
    if len(pts) == 0:
        return np.zeros((NCLS, rows * cols), np.float32)
    if polar:
        return oracle.raster_polar(pts, res, ang, _lut(), NCLS, rows, cols)
    return oracle.raster_cart(pts, res, _lut(), NCLS, rows, cols)


def _raster(k, polar, pts, res, ang, rows, cols, ws):
    """img, pk of tdr_k_raster_polar / _cart with the key workspace at `ws` (a device address or None)."""
    import torch
    n = len(pts)
    dev = k.to_device(pts if n else np.zeros((1, 4), np.float32))
    lut = k.to_device(_lut())
    rf = int(k.lib.tdr_rec_floats(NCLS))
    img = torch.full((NCLS, rows * cols), -7.0, device=k.device)   # the tiles write every cell, zeros included
    pk = torch.full((rows * cols * rf,), -7.0, device=k.device)
    wsp = C.c_void_p(ws) if ws is not None else None
    if polar:
        rc = k.lib.tdr_k_raster_polar(C.c_void_p(dev.data_ptr()), 4, 3, n, C.c_float(res), C.c_float(ang),
                                      C.c_void_p(lut.data_ptr()), NCLS, rows, cols, C.c_void_p(img.data_ptr()),
                                      C.c_void_p(pk.data_ptr()), wsp, k.stream())
    else:
        rc = k.lib.tdr_k_raster_cart(C.c_void_p(dev.data_ptr()), 4, 3, n, C.c_float(res), C.c_void_p(lut.data_ptr()), NCLS,
                                     rows, cols, C.c_void_p(img.data_ptr()), C.c_void_p(pk.data_ptr()), wsp, k.stream())
    assert rc == 0, k.lib.tdr_last_error().decode()
    k.synchronize()
    return img.cpu().numpy(), pk.cpu().numpy()


def _geometry(polar, rows, cols):
    """(res, ang_res, spread): a cloud of half-width `spread` covers the image and reaches beyond it."""
    if polar:
        return 0.5, float(np.float32(2 * np.pi / rows)), 0.5 * cols
    return 0.5, 1.0, 0.25 * min(rows, cols)


@pytest.mark.parametrize("polar", [1, 0], ids=["polar", "cart"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_count_every_shape_aligned_and_not(k, oracle, polar, shape):
    """n = 0, 3, 4, 5, 4099, 20 483 points into every image shape, the key workspace once 16-byte aligned and once 4 bytes past
    such an address (the scalar head), and once absent (the tiles of the form without keys)."""
    import torch
    rows, cols = shape
    res, ang, spread = _geometry(polar, rows, cols)
    rng = np.random.default_rng(7000 + 10 * rows + cols + polar)
    wsbuf = torch.zeros(4 * max(COUNTS) + 64, dtype=torch.uint8, device=k.device)
    base = (wsbuf.data_ptr() + 15) & ~15
    for n in COUNTS:
        pts = _cloud(rng, n, spread)
        ref = _oracle(oracle, polar, pts, res, ang, rows, cols)
        if n >= 4099:
            assert ref.sum() > n // 4 and ref.sum() < n   # most points land, some do not
        for ws in (base, base + 4, base + 8, base + 12, None):
            img, pk = _raster(k, polar, pts, res, ang, rows, cols, ws)
            assert np.array_equal(img, ref), (n, ws is None or ws - base)
            assert np.array_equal(pk, _records(k, ref, rows, cols)), (n, ws is None or ws - base)


@pytest.mark.parametrize("polar", [1, 0], ids=["polar", "cart"])
def test_one_bin_and_no_bin(k, oracle, polar):
    """Every point in one bin (4099 atomics on one counter of one tile) and points that map to no bin at all (beyond the
    image, or of no class): the images are the oracle's — one cell of 4099, and zeros."""
    import torch
    rows, cols = 100, 25
    res, ang, _ = _geometry(polar, rows, cols)
    n = 4099
    ws = torch.zeros(4 * n + 16, dtype=torch.uint8, device=k.device)
    one = np.zeros((n, 4), np.float32)
    one[:, 0], one[:, 1], one[:, 3] = 3.2, 1.1, 2.0
    ref = _oracle(oracle, polar, one, res, ang, rows, cols)
    assert ref.max() == n and np.count_nonzero(ref) == 1
    img, pk = _raster(k, polar, one, res, ang, rows, cols, ws.data_ptr())
    assert np.array_equal(img, ref) and np.array_equal(pk, _records(k, ref, rows, cols))
    rng = np.random.default_rng(71)
    none = np.zeros((n, 4), np.float32)
    ang_pt = rng.random(n) * 2 * np.pi
    far = 10.0 * max(rows, cols)   # beyond the image in either geometry
    none[:, 0], none[:, 1] = far * np.cos(ang_pt), far * np.sin(ang_pt)
    none[:, 3] = rng.integers(1, NCLS + 1, n)
    none[: n // 2, :2] = rng.normal(0, 2, (n // 2, 2))   # inside the image, but of no class
    none[: n // 2, 3] = 0.0
    ref = _oracle(oracle, polar, none, res, ang, rows, cols)
    assert ref.sum() == 0
    img, pk = _raster(k, polar, none, res, ang, rows, cols, ws.data_ptr())
    assert np.array_equal(img, ref) and np.array_equal(pk, _records(k, ref, rows, cols))


def test_batched_renderer_two_scans_of_different_length(k, oracle):
    """tdr_batch_render_polar shares the tile bodies and the launch shape: two clouds of different length (4099 and 5 points,
    then swapped, on the renderers' reused buffers) give the oracle's images."""
    from top_down_renderer_amd import batch
    rng = np.random.default_rng(72)
    rows, cols = 100, 25
    ang = float(np.float32(2 * np.pi / rows))
    rs = [batch.Renderer(_lut()), batch.Renderer(_lut())]
    for counts in ((4099, 5), (5, 4099)):
        clouds = [(_cloud(rng, n, 0.5 * cols), 4, 3) for n in counts]
        res = [0.5, 0.8]
        batch.render_batch(rs, clouds, res, ang, NCLS, rows, cols)
        for r, (pts, _, _), rr in zip(rs, clouds, res):
            ref = oracle.raster_polar(pts, rr, ang, _lut(), NCLS, rows, cols)
            img, pk = r.get_render()   # img (ncls, rows, cols); the oracle's planes are column-major: cell row + rows * col
            assert np.array_equal(np.transpose(img, (0, 2, 1)).reshape(NCLS, -1), ref)
            assert np.array_equal(np.asarray(pk, np.float32).reshape(-1), _records(k, ref, rows, cols))
