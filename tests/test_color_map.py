"""The static colour raster map (include/tdr.h: tdr_png_read_color_host, tdr_k_color_index, tdr_k_map_from_color,
tdr_map_load_color_image, tdr_map_load_color_png): the host PNG reader against PIL-written fixtures
(tests/golden/png/, expected images in tests/golden/png_bgr.npz, written by tests/golden/make_png_golden.py) and against
an in-test NumPy encoder of known samples (every colour type, bit depth, interlace method and filter type), the reader's
defences, the argument checks; on the GPU, color2Ind against NumPy and the colour path against the label path, the
raster-cache path and the SVG path, the C++ façade and the Python TopDownMap.
"""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

from top_down_renderer_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PNG_DIR = os.path.join(ROOT, "tests", "golden", "png")
GOLDEN = os.path.join(ROOT, "tests", "golden", "png_bgr.npz")
vp = C.c_void_p


def lib():
    build.build()
    return _lib.load()


def read(path):
    from top_down_renderer_amd.kernels import png_read_color
    build.build()
    return png_read_color(path)


def read_rc(path, cap=None):
    """(rc, message, w, h, image or None) of tdr_png_read_color_host with a buffer of `cap` bytes (None: size query)."""
    L = lib()
    w, h = C.c_int(0), C.c_int(0)
    buf = np.zeros(max(cap or 0, 1), np.uint8)
    rc = L.tdr_png_read_color_host(str(path).encode(), buf.ctypes.data_as(vp) if cap is not None else None,
                                   cap or 0, C.byref(w), C.byref(h))
    return rc, L.tdr_last_error().decode(), w.value, h.value, buf


# ---- an in-test PNG encoder of known samples --------------------------------------------------------------------------
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}


def chunk(t, d=b""):
    t = t.encode() if isinstance(t, str) else t
    return len(d).to_bytes(4, "big") + t + d + (zlib.crc32(t + d) & 0xFFFFFFFF).to_bytes(4, "big")


def pack_rows(s, depth):
    """(h, w, nch) samples -> (h, row_bytes) uint8, sub-byte samples from the most significant bit, 16 bits big-endian."""
    h = s.shape[0]
    flat = s.reshape(h, -1).astype(np.uint32)
    if depth == 16:
        return np.stack([flat >> 8, flat & 0xFF], axis=2).reshape(h, -1).astype(np.uint8)
    if depth == 8:
        return flat.astype(np.uint8)
    bits = np.unpackbits(flat.astype(np.uint8)[..., None], axis=2)[..., 8 - depth:].reshape(h, -1)
    return np.packbits(bits, axis=1)


def filter_rows(raw, bpp, ftypes):
    """PNG filtering of unfiltered rows raw (h, n) with per-row filter types; every prediction comes from raw bytes."""
    h, n = raw.shape
    r = raw.astype(np.int32)
    out = np.empty((h, n + 1), np.uint8)
    for y in range(h):
        a = np.r_[np.zeros(bpp, np.int32), r[y, :-bpp]] if n > bpp else np.zeros(n, np.int32)
        a = a[:n]
        b = r[y - 1] if y else np.zeros(n, np.int32)
        c = (np.r_[np.zeros(bpp, np.int32), r[y - 1, :-bpp]][:n] if y else np.zeros(n, np.int32)) if n > bpp else \
            np.zeros(n, np.int32)
        ft = int(ftypes[y % len(ftypes)])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out[y, 0] = ft
        out[y, 1:] = ((r[y] - pred) & 0xFF).astype(np.uint8)
    return out


def encode(samples, ctype, depth, interlace=0, ftypes=(0, 1, 2, 3, 4), palette=None, idat_pieces=1, ancillary=(),
           level=6, plte_after_idat=False, drop_plte=False, extra_chunks=()):
    """PNG bytes of samples (h, w, nch) in colour type ctype / bit depth depth."""
    h, w = samples.shape[:2]
    nch = CHANNELS[ctype]
    bpp = max(1, nch * depth // 8)
    stream = []
    passes = ADAM7 if interlace else [(0, 0, 1, 1)]
    for x0, y0, dx, dy in passes:
        sub = samples[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        stream.append(filter_rows(pack_rows(sub, depth), bpp, ftypes).tobytes())
    z = zlib.compress(b"".join(stream), level)
    cuts = sorted(set([0, len(z)] + [int(c) for c in np.linspace(0, len(z), idat_pieces + 1)[1:-1]]))
    idats = [chunk("IDAT", z[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    hdr = w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([depth, ctype, 0, 0, interlace])
    out = b"\x89PNG\r\n\x1a\n" + chunk("IHDR", hdr)
    pre = [c for c in ancillary if c[0] != "after"]
    post = [c for c in ancillary if c[0] == "after"]
    for _, t, d in pre:
        out += chunk(t, d)
    plte = chunk("PLTE", np.asarray(palette, np.uint8).tobytes()) if palette is not None and not drop_plte else b""
    if not plte_after_idat:
        out += plte
    out += b"".join(idats)
    if plte_after_idat:
        out += plte
    for t, d in extra_chunks:
        out += chunk(t, d)
    for _, t, d in post:
        out += chunk(t, d)
    return out + chunk("IEND")


def expected_bgr(samples, ctype, depth, palette=None):
    """The conversion rules of cv::imread (IMREAD_COLOR) over libpng, restated."""
    s = samples.astype(np.int64)
    if depth == 16:
        s = s >> 8                                                   # png_set_strip_16
    if ctype in (0, 4):
        g = s[..., 0] * (255 // ((1 << depth) - 1)) if depth < 8 else s[..., 0]   # expand_gray_1_2_4_to_8; alpha dropped
        return np.repeat(g[..., None], 3, axis=2).astype(np.uint8)
    if ctype == 3:
        pal = np.zeros((256, 3), np.uint8)                           # an index past the palette: black
        pal[:len(palette)] = palette
        return pal[s[..., 0]][..., ::-1].astype(np.uint8)
    return s[..., 2::-1].astype(np.uint8)                            # RGB(A) -> B, G, R; alpha dropped


def random_samples(rng, h, w, ctype, depth, n_pal=None):
    hi = (n_pal if ctype == 3 and n_pal else 1 << depth)
    return rng.integers(0, hi, (h, w, CHANNELS[ctype])).astype(np.uint32)


ANC = (("pre", "gAMA", (45455).to_bytes(4, "big")), ("pre", "tEXt", b"Comment\x00colour map"),
       ("pre", "eXIf", b"MM\x00*\x00\x00\x00\x08\x00\x00"), ("after", "tEXt", b"Author\x00test"))


# ---- CPU: the reader ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(PNG_DIR) if f.endswith(".png")))
def test_reader_matches_pil_fixtures(name):
    got = read(os.path.join(PNG_DIR, name + ".png"))
    assert np.array_equal(got, np.load(GOLDEN)[name])


CASES = [(ct, d, il) for ct in (0, 2, 3, 4, 6) for d in DEPTHS[ct] for il in (0, 1)]


@pytest.mark.parametrize("ctype,depth,interlace", CASES)
def test_reader_matches_encoded_samples(tmp_path, ctype, depth, interlace):
    """Every colour type x bit depth x interlace method, every filter type (per row, in turn and at random), split IDAT,
    ancillary chunks (tRNS, gAMA, tEXt, eXIf) without effect, on odd sizes down to 1 x 1."""
    rng = np.random.default_rng(1000 * ctype + 10 * depth + interlace)
    for k, (h, w) in enumerate([(1, 1), (1, 9), (7, 1), (5, 13), (11, 3), (17, 29), (9, 64)]):
        n_pal = None
        palette = None
        if ctype == 3:
            n_pal = int(rng.integers(1, (1 << depth) + 1))
            palette = rng.integers(0, 256, (n_pal, 3)).astype(np.uint8)
        s = random_samples(rng, h, w, ctype, depth, n_pal)
        ftypes = [k % 5] if k < 5 else list(rng.integers(0, 5, 8))
        anc = list(ANC)
        if ctype == 3:
            anc.insert(0, ("pre", "tRNS", bytes(rng.integers(0, 256, n_pal).astype(np.uint8))))
        elif ctype in (0, 2):
            anc.insert(0, ("pre", "tRNS", b"\x00\x01" * (1 if ctype == 0 else 3)))
        data = encode(s, ctype, depth, interlace, ftypes, palette, idat_pieces=1 + k % 4, ancillary=anc)
        p = tmp_path / f"c{k}.png"
        p.write_bytes(data)
        got = read(p)
        assert np.array_equal(got, expected_bgr(s, ctype, depth, palette)), (h, w, ftypes)
        if ctype == 2 and depth == 8 and not interlace and k % 2:   # PIL agrees with cv::imread on 8-bit colour
            try:
                from PIL import Image
            except ImportError:
                continue
            assert np.array_equal(got, np.asarray(Image.open(p).convert("RGB"))[..., ::-1])


def test_reader_palette_index_past_the_palette_is_black(tmp_path):
    s = np.array([[[0], [1], [2], [3]]], np.uint32)
    pal = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)
    (tmp_path / "p.png").write_bytes(encode(s, 3, 2, palette=pal))
    got = read(tmp_path / "p.png")
    assert got[0].tolist() == [[30, 20, 10], [60, 50, 40], [0, 0, 0], [0, 0, 0]]


def test_reader_is_defensive(tmp_path):
    """Each refusal: rc -1 and a message that starts with "png" and names the problem."""
    rng = np.random.default_rng(5)
    s = random_samples(rng, 6, 7, 2, 8)
    good = encode(s, 2, 8)
    (tmp_path / "good.png").write_bytes(good)
    rc, msg, w, h, _ = read_rc(tmp_path / "good.png")              # size query: the size, and -1 (no buffer)
    assert rc == -1 and (w, h) == (7, 6) and msg.startswith("png") and "needs 126 bytes" in msg
    rc, msg, w, h, buf = read_rc(tmp_path / "good.png", cap=125)    # too small: the size is still reported
    assert rc == -1 and (w, h) == (7, 6) and "needs" in msg
    rc, msg, w, h, buf = read_rc(tmp_path / "good.png", cap=126)
    assert rc == 0 and np.array_equal(buf.reshape(6, 7, 3), expected_bgr(s, 2, 8))

    def refused(data, words, name="bad.png"):
        (tmp_path / name).write_bytes(data)
        rc, msg, *_ = read_rc(tmp_path / name, cap=1 << 20)
        assert rc == -1 and msg.startswith("png") and all(wd in msg for wd in words), msg

    bad = bytearray(good)
    bad[40] ^= 0x01                                                 # inside IDAT's data
    refused(bytes(bad), ["CRC"])
    for cut in (10, 33, 45, len(good) - 13, len(good) - 1):        # truncation, IEND missing included
        refused(good[:cut], ["truncated"])
    pal = rng.integers(0, 256, (4, 3)).astype(np.uint8)
    sp = random_samples(rng, 6, 7, 3, 2, 4)
    refused(encode(sp, 3, 2, palette=pal, drop_plte=True), ["PLTE", "missing"])
    refused(encode(s, 2, 8, palette=pal, plte_after_idat=True), ["PLTE", "misplaced"])
    refused(encode(s, 2, 8, extra_chunks=[("ZZZZ", b"abc")]), ["critical", "ZZZZ"])
    # a header that announces 2^24 x 2^24 pixels over a few bytes of image data: refused before allocating
    z = zlib.compress(b"\x00" * 64)
    bomb = (b"\x89PNG\r\n\x1a\n" + chunk("IHDR", (1 << 24).to_bytes(4, "big") * 2 + bytes([8, 2, 0, 0, 0])) +
            chunk("IDAT", z) + chunk("IEND"))
    refused(bomb, ["announces"])
    # short image data and a broken deflate stream
    refused(b"\x89PNG\r\n\x1a\n" + chunk("IHDR", good[16:29]) + chunk("IDAT", zlib.compress(b"\x00" * 20)) +
            chunk("IEND"), ["inflate"])
    refused(encode(s, 2, 8, level=0)[:60], ["truncated"])
    refused(b"not a png at all", ["not a PNG"])
    refused(b"\x89PNG\r\n\x1a\n" + chunk("IHDR", (7).to_bytes(4, "big") * 2 + bytes([4, 2, 0, 0, 0])) + chunk("IEND"),
            ["invalid header"])
    rc, msg, *_ = read_rc(tmp_path / "missing.png", cap=100)
    assert rc == -1 and msg.startswith("png") and "cannot open" in msg
    L = lib()
    assert L.tdr_png_read_color_host(None, None, 0, None, None) == -1 and "null" in L.tdr_last_error().decode()


def test_abi_validation():
    """Every argument is checked before any device work (the map handle is checked last: NULL here, no GPU needed)."""
    L = lib()
    P = lambda a: a.ctypes.data_as(vp)
    img = np.zeros((10, 12, 3), np.uint8)
    keys = np.zeros(3, np.uint32)
    lut = np.zeros(3, np.int32)

    def li(bgr=P(img), h=10, w=12, keys_=P(keys), lut_=P(lut), n=3, ncls=3, res=1.0):
        rc = L.tdr_map_load_color_image(None, bgr, h, w, keys_, lut_, n, ncls, C.c_float(res), 0, 0)
        return rc, L.tdr_last_error().decode()
    assert li()[0] == -1 and "null map" in li()[1]
    for kw, msg in ((dict(bgr=None), "null image"), (dict(keys_=None), "null lookup"), (dict(lut_=None), "null lookup"),
                    (dict(n=0), "lut_size"), (dict(n=257), "lut_size"), (dict(ncls=0), "num_classes"),
                    (dict(ncls=16), "num_classes"), (dict(res=0.0), "resolution"), (dict(res=-1.0), "resolution"),
                    (dict(res=float("nan")), "resolution"), (dict(res=0.19), "resolution"), (dict(h=0), "size"),
                    (dict(w=-1), "size"), (dict(h=1 << 25), "size"), (dict(res=20.0), "empty map")):
        rc, err = li(**kw)
        assert rc == -1 and msg in err, (kw, err)
    assert li(res=0.2)[1].find("resolution") < 0                  # 0.2 is allowed: a 250-cell window

    def lp(path=os.path.join(PNG_DIR, "rgb.png").encode(), keys_=P(keys), lut_=P(lut), n=3, ncls=3, res=1.0):
        rc = L.tdr_map_load_color_png(None, path, keys_, lut_, n, ncls, C.c_float(res), 0, 0)
        return rc, L.tdr_last_error().decode()
    assert lp()[0] == -1 and "null map" in lp()[1]
    for kw, msg in ((dict(path=None), "null path"), (dict(keys_=None), "null lookup"), (dict(n=300), "lut_size"),
                    (dict(ncls=0), "num_classes"), (dict(res=0.0), "resolution")):
        rc, err = lp(**kw)
        assert rc == -1 and msg in err, (kw, err)
    out = np.zeros(120, np.uint8)

    def ci(bgr=P(img), h=10, w=12, keys_=P(keys), n=3, o=P(out)):
        rc = L.tdr_k_color_index(bgr, h, w, keys_, n, o, None)
        return rc, L.tdr_last_error().decode()
    for kw, msg in ((dict(bgr=None), "null"), (dict(keys_=None), "null"), (dict(o=None), "null"), (dict(n=0), "keys"),
                    (dict(n=257), "keys"), (dict(h=0), "size")):
        rc, err = ci(**kw)
        assert rc == -1 and msg in err, (kw, err)
    ws = np.zeros(16, np.uint8)
    rec = np.zeros(16, np.float32)

    def mc(bgr=P(img), keys_=P(keys), lut_=P(lut), n=3, ncls=3, res=1.0):
        rc = L.tdr_k_map_from_color(bgr, 10, 12, keys_, lut_, n, ncls, C.c_float(res), P(rec), P(ws), None)
        return rc, L.tdr_last_error().decode()
    for kw, msg in ((dict(bgr=None), "null"), (dict(lut_=None), "null"), (dict(n=257), "lut size"),
                    (dict(ncls=16), "class count"), (dict(res=0.1), "window")):
        rc, err = mc(**kw)
        assert rc == -1 and msg in err, (kw, err)


def test_color_key_convention():
    from top_down_renderer_amd.top_down_map import color_key, svg_fill_key
    assert color_key((0, 0, 255)) == 0x0000FF == svg_fill_key((0, 0, 255))   # RGB (255, 0, 0) in BGR order
    img = np.array([[[1, 2, 3], [255, 0, 0]]], np.uint8)
    assert color_key(img).tolist() == [[0x010203, 0xFF0000]]


# ---- NumPy restatements -------------------------------------------------------------------------------------------
def np_color2ind(bgr, keys):
    """color2Ind as the exact inverse of ind2Color: the smallest index with the pixel's key, 255 where none matches."""
    from top_down_renderer_amd.top_down_map import color_key
    k = color_key(bgr)
    out = np.full(k.shape, 255, np.uint8)
    for i in range(len(keys) - 1, -1, -1):                         # downwards: the smallest index is written last
        out[k == (int(keys[i]) & 0xFFFFFF)] = i
    return out


def palette_image(rng, h, w, colours, p_unmatched=0.1):
    """A random colour map: blobs of the table's colours, some pixels of colours outside the table."""
    coarse = rng.integers(0, len(colours), (h // 4 + 2, w // 4 + 2))
    idx = np.repeat(np.repeat(coarse, 4, 0), 4, 1)[:h, :w]
    idx = np.where(rng.random((h, w)) < 0.05, rng.integers(0, len(colours), (h, w)), idx)
    img = np.asarray(colours, np.uint8)[idx]
    stray = rng.random((h, w)) < p_unmatched
    img[stray] = rng.integers(0, 256, (int(stray.sum()), 3)).astype(np.uint8)
    return img


def key_table(rng, n, dup=True):
    """n fill keys (with key 0 and a few duplicates) and the BGR colours that carry them."""
    keys = rng.choice(1 << 24, n, replace=False).astype(np.uint32)
    keys[0] = 0
    if dup and n > 4:
        keys[n - 1] = keys[1]
        keys[n - 2] = keys[2]
    bgr = np.stack([(keys >> 16) & 0xFF, (keys >> 8) & 0xFF, keys & 0xFF], 1).astype(np.uint8)
    return keys, bgr


def test_restatement_of_color2ind():
    keys = np.array([0x0000FF, 0x00FF00, 0x0000FF, 0x123456], np.uint32)
    img = np.array([[[0, 0, 255], [0, 255, 0], [0x12, 0x34, 0x56], [255, 0, 0], [0, 0, 0]]], np.uint8)
    assert np_color2ind(img, keys).tolist() == [[0, 1, 3, 255, 255]]


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kern():
    from top_down_renderer_amd.kernels import HipKernels
    return HipKernels()


@pytest.fixture()
def handle(kern):
    from top_down_renderer_amd._lib import check
    m = vp()
    check(kern.lib.tdr_map_create(C.byref(m)))
    yield m
    kern.lib.tdr_map_destroy(m)


def new_handle(kern):
    from top_down_renderer_amd._lib import check
    m = vp()
    check(kern.lib.tdr_map_create(C.byref(m)))
    return m


def cache_of(kern, m, d, ncls):
    """Everything the map cache holds (class maps, mask, geometric layers), read back through tdr_map_save_cache."""
    from top_down_renderer_amd import eig_io
    from top_down_renderer_amd._lib import check
    check(kern.lib.tdr_map_save_cache(m, str(d).encode(), b"m"))
    out = [eig_io.read_eig(str(d / f"class_map{c}.eig"), np.float32) for c in range(ncls)]
    out.append(eig_io.read_eig(str(d / "class_mask.eig"), np.uint8))
    out += [eig_io.read_eig(str(d / f"geo_map{c}.eig"), np.float32) for c in range(2)]
    return out


def map_info(kern, m):
    ncls, rows, cols, have = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    kern.lib.tdr_map_info(m, C.byref(ncls), C.byref(rows), C.byref(cols), None, C.byref(have))
    return ncls.value, rows.value, cols.value, have.value


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(8))
def test_gpu_color_index_matches_numpy(kern, case):
    rng = np.random.default_rng(40 + case)
    n = [1, 2, 7, 64, 255, 256, 256, 100][case]
    h, w = [(1, 1), (3, 5), (17, 33), (64, 48), (101, 77), (128, 256), (5, 3), (31, 16)][case]
    keys, cols_ = key_table(rng, n)
    img = palette_image(rng, h, w, cols_, p_unmatched=0.2)
    got = kern.color_index(img, keys)
    assert np.array_equal(got, np_color2ind(img, keys))
    if case == 6:   # an unaligned device image takes the per-pixel path
        import torch
        buf = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device=kern.device)
        buf[1:] = torch.from_numpy(img.reshape(-1)).to(kern.device)
        got2 = kern.color_index(buf[1:].view(h, w, 3), keys).cpu().numpy()
        assert np.array_equal(got2, np_color2ind(img, keys))


SHAPES = [(64, 64, 1.0), (61, 77, 1.0), (48, 160, 1.0), (33, 47, 0.5), (40, 64, 2.0), (71, 53, 1.7), (1, 16, 1.0),
          (16, 1, 1.0), (9, 200, 0.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,res", SHAPES)
def test_gpu_color_path_equals_label_path(kern, tmp_path, h, w, res):
    """tdr_map_load_color_image == color2Ind (NumPy) + tdr_map_set_labels, bit for bit: class maps, mask, records
    (plain and compact); and the NumPy oracle of loadCompressedRasterMap + computeDists."""
    from oracle import np_oracle
    rng = np.random.default_rng(h * 1000 + w)
    ncls = 5
    keys, cols_ = key_table(rng, 12)
    lut = np.array([0, 1, 2, 3, 4, 1, 7, -1, 2, 3, 0, 4], np.int32)     # 7 / -1: no class
    img = palette_image(rng, h, w, cols_)
    labels = np_color2ind(img, keys)
    a, b = new_handle(kern), new_handle(kern)
    try:
        kern.map_load_color_image(a, img, keys, lut, ncls, res)
        from top_down_renderer_amd._lib import check
        check(kern.lib.tdr_map_set_labels(b, labels.ctypes.data_as(vp), h, w, lut.ctypes.data_as(vp), len(lut), ncls,
                                          C.c_float(res), 0, 0))
        ca, cb = cache_of(kern, a, tmp_path / "a", ncls), cache_of(kern, b, tmp_path / "b", ncls)
        for x, y in zip(ca[:ncls + 1], cb[:ncls + 1]):
            assert np.array_equal(x, y)
        assert map_info(kern, a)[3] == 1
    finally:
        kern.lib.tdr_map_destroy(a)
        kern.lib.tdr_map_destroy(b)
    ma = kern.make_map_from_color(img, keys, lut, ncls, res)
    mb = kern.make_map_from_labels(labels, lut, ncls, res)
    assert np.array_equal(ma.rec.cpu().numpy(), mb.rec.cpu().numpy())
    assert (ma.desc.cwords, ma.desc.dict_n) == (mb.desc.cwords, mb.desc.dict_n)
    if ma.crec is not None:   # the compact records, decoded (their padding words are never written)
        from top_down_renderer_amd.kernels import _ptr
        dec = []
        for m in (ma, mb):
            out = kern.empty(tuple(m.rec.shape))
            _lib.check(kern.lib.tdr_k_unpack_compact_map(C.byref(m.desc), _ptr(out), kern.stream()))
            dec.append(out.cpu().numpy())
        assert np.array_equal(dec[0], dec[1])
        assert np.array_equal(ma.dict.cpu().numpy()[:ma.desc.dict_n], mb.dict.cpu().numpy()[:mb.desc.dict_n])
    maps, mask = np_oracle.load_compressed_raster_map(labels, lut, ncls, res)
    assert np.array_equal(ca[ncls], mask)                           # [row, col]
    for c in range(ncls):
        assert np.array_equal(ca[c], maps[c])


def class_grid(img, keys, lut, ncls, res):
    """The flattened class of every map cell (yi = 0 at the bottom), -1 unknown: loadCompressedRasterMap's sampling."""
    labels = np_color2ind(img, keys).astype(np.int64)
    h, w = labels.shape
    f = np.float32
    rows, cols = int(f(h) / f(res)), int(f(w) / f(res))
    iy = np.maximum((f(h) - np.arange(rows).astype(f) * f(res) - f(1)).astype(f).astype(np.int64), 0)
    ix = np.minimum((np.arange(cols).astype(f) * f(res)).astype(f).astype(np.int64), w - 1)
    lab = labels[iy[:, None], ix[None, :]]
    lut = np.asarray(lut, np.int64)
    c = np.where(lab < len(lut), lut[np.minimum(lab, len(lut) - 1)], -1)
    return np.where((c >= 0) & (c < ncls), c, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,res", [(64, 80, 1.0), (57, 43, 1.0), (60, 90, 2.0)])
@pytest.mark.parametrize("road", [True, False])
def test_gpu_color_path_equals_raster_cache_path(kern, tmp_path, h, w, res, road):
    """The class planes of the colour map written as a raster-cache directory and loaded with tdr_map_load_rasters give
    the same map, geometric layers included; have_map is true even without road; getClassesAtPoint agrees."""
    from top_down_renderer_amd._lib import check
    rng = np.random.default_rng(h + w + int(road))
    ncls = 5
    keys, cols_ = key_table(rng, 8, dup=False)
    lut = np.array([0, 1, 2, 3, 4, 3, 4, 2], np.int32)
    if not road:
        lut[lut == 1] = 0
    img = palette_image(rng, h, w, cols_)
    grid = class_grid(img, keys, lut, ncls, res)
    rows, cols = grid.shape
    d = tmp_path / "rc"
    d.mkdir()
    for c in range(ncls):   # stored like saveRasterizedMaps: row 0 = the top of the map
        kern.png_write_gray8(str(d / f"class{c}.png"), np.where(grid == c, 0, 255).astype(np.uint8)[::-1])
    a, b = new_handle(kern), new_handle(kern)
    try:
        kern.map_load_color_image(a, img, keys, lut, ncls, res)
        check(kern.lib.tdr_map_load_rasters(b, str(d).encode(), ncls, C.c_float(res), 0, 0))
        assert map_info(kern, a) == map_info(kern, b) == (ncls, rows, cols, 1)
        ca, cb = cache_of(kern, a, tmp_path / "a", ncls), cache_of(kern, b, tmp_path / "b", ncls)
        for x, y in zip(ca, cb):
            assert np.array_equal(x, y)
        assert (ca[-1] == 0).any() and (ca[-2] == 0).any()             # derived, not the constant 1 of updateMap
        for _ in range(40):
            px, py = int(rng.integers(0, cols)), int(rng.integers(0, rows))
            ba, bb = C.c_uint32(0), C.c_uint32(0)
            check(kern.lib.tdr_map_classes_at_point(a, px, py, C.byref(ba)))
            check(kern.lib.tdr_map_classes_at_point(b, px, py, C.byref(bb)))
            assert ba.value == bb.value
    finally:
        kern.lib.tdr_map_destroy(a)
        kern.lib.tdr_map_destroy(b)


@pytest.mark.gpu
def test_gpu_svg_and_png_agree_on_the_key_convention(kern, tmp_path):
    """One scene of axis-aligned integer rectangles as an SVG and as an RGB PNG, one colour table: every cell whose 3 x 3
    neighbourhood is uniform gets the same class on both paths (guards the B, G, R order of the keys)."""
    from top_down_renderer_amd.top_down_map import color_key
    rng = np.random.default_rng(3)
    W, H, ncls = 120, 90, 4
    rgb = np.array([[255, 0, 0], [0, 128, 0], [0, 0, 255], [200, 100, 50], [10, 20, 30]], np.uint8)   # R, G, B
    keys = np.array([color_key(c[::-1]) for c in rgb], np.uint32)
    lut = np.array([0, 1, 2, 3, 1], np.int32)
    img = np.full((H, W, 3), 255, np.uint8)   # white: no class
    rects = ['<svg xmlns="http://www.w3.org/2000/svg" width="%d" height="%d">' % (W, H)]
    for gy in range(0, H, 15):        # one rectangle per 20 x 15 tile at most: no overlaps (an SVG cell may hold several
        for gx in range(0, W, 20):    # classes where shapes overlap, a PNG pixel one colour)
            if rng.random() < 0.2:
                continue
            x, y = gx + int(rng.integers(0, 5)), gy + int(rng.integers(0, 4))
            w, h = int(rng.integers(6, 20 - (x - gx) + 1)), int(rng.integers(5, 15 - (y - gy) + 1))
            k = int(rng.integers(0, len(rgb)))
            img[y:y + h, x:x + w] = rgb[k]
            rects.append('<rect x="%d" y="%d" width="%d" height="%d" fill="#%02x%02x%02x"/>' % (x, y, w, h, *rgb[k]))
    (tmp_path / "s.svg").write_text("\n".join(rects + ["</svg>"]))
    (tmp_path / "s.png").write_bytes(encode(img.astype(np.uint32), 2, 8))
    a, b = new_handle(kern), new_handle(kern)
    try:
        kern.map_load_svg(a, str(tmp_path / "s.svg"), keys, lut, ncls, [], 1.0)
        kern.map_load_color_png(b, str(tmp_path / "s.png"), keys, lut, ncls, 1.0)
        ca, cb = cache_of(kern, a, tmp_path / "a", ncls), cache_of(kern, b, tmp_path / "b", ncls)
    finally:
        kern.lib.tdr_map_destroy(a)
        kern.lib.tdr_map_destroy(b)

    def classes(cache):   # (rows, cols) class index of each known cell, -1 unknown
        inside = np.stack([(cache[c] == 0) & (cache[ncls] == 0) for c in range(ncls)])
        return np.where(inside.any(0), inside.argmax(0), -1)
    sa, sb = classes(ca), classes(cb)
    assert sa.shape == sb.shape == (H, W)
    pad = np.pad(sb, 1, mode="edge")
    uniform = np.ones_like(sb, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            uniform &= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == sb
    assert uniform.sum() > 0.5 * H * W and (sb[uniform] >= 0).sum() > 0.1 * H * W
    assert np.array_equal(sa[uniform], sb[uniform])


@pytest.mark.gpu
def test_gpu_full_size_png(kern, tmp_path):
    """A 4000 x 4000 colour PNG through tdr_map_load_color_png equals its label image through tdr_map_set_labels."""
    from top_down_renderer_amd._lib import check
    rng = np.random.default_rng(11)
    keys, cols_ = key_table(rng, 10)
    lut = np.array([0, 1, 2, 3, 4, 5, 1, 2, -1, 5], np.int32)
    ncls, H, W = 6, 4000, 4000
    coarse = rng.integers(0, len(cols_), (H // 16, W // 16))
    img = np.asarray(cols_, np.uint8)[np.repeat(np.repeat(coarse, 16, 0), 16, 1)]
    img[rng.random((H, W)) < 0.01] = (1, 2, 3)                        # unmatched colour
    (tmp_path / "big.png").write_bytes(encode(img[..., ::-1].astype(np.uint32), 2, 8, ftypes=(4, 1, 2), idat_pieces=7))
    assert np.array_equal(read(tmp_path / "big.png"), img)
    labels = np_color2ind(img, keys)
    a, b = new_handle(kern), new_handle(kern)
    try:
        kern.map_load_color_png(a, str(tmp_path / "big.png"), keys, lut, ncls, 1.0)
        check(kern.lib.tdr_map_set_labels(b, labels.ctypes.data_as(vp), H, W, lut.ctypes.data_as(vp), len(lut), ncls,
                                          C.c_float(1.0), 0, 0))
        ca, cb = cache_of(kern, a, tmp_path / "a", ncls), cache_of(kern, b, tmp_path / "b", ncls)
        for x, y in zip(ca[:ncls + 1], cb[:ncls + 1]):
            assert np.array_equal(x, y)
    finally:
        kern.lib.tdr_map_destroy(a)
        kern.lib.tdr_map_destroy(b)


@pytest.mark.gpu
def test_gpu_failed_load_leaves_the_handle(kern, handle, tmp_path):
    rng = np.random.default_rng(2)
    keys, cols_ = key_table(rng, 6, dup=False)
    lut = np.arange(6, dtype=np.int32) % 3
    img = palette_image(rng, 40, 50, cols_)
    kern.map_load_color_image(handle, img, keys, lut, 3, 1.0)
    before = cache_of(kern, handle, tmp_path / "a", 3)
    (tmp_path / "bad.png").write_bytes(encode(img[..., ::-1].astype(np.uint32), 2, 8)[:-20])
    with pytest.raises(_lib.TdrError, match="png"):
        kern.map_load_color_png(handle, str(tmp_path / "bad.png"), keys, lut, 3, 1.0)
    with pytest.raises(_lib.TdrError, match="resolution"):
        kern.map_load_color_image(handle, img[:20], keys, lut, 3, 0.1)
    assert map_info(kern, handle) == (3, 40, 50, 1)
    for x, y in zip(before, cache_of(kern, handle, tmp_path / "b", 3)):
        assert np.array_equal(x, y)


FACADE_RGB = [(255, 0, 0), (0, 128, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0), (128, 128, 128)]   # LUT indices 0..5


@pytest.mark.gpu
def test_facade_color_png_constructor_and_python_path(kern, tmp_path):
    """tests/cpp/facade_color_png.cpp: TopDownMap(params) with a .png map_path — decode, colour lookup, distance maps,
    the map cache and no raster cache; the second construction hits the cache; a corrupt PNG leaves the map empty and
    writes nothing; a .jpg stays empty with a message that points to the BGR entry point.  The Python
    loadColorRasterMap builds the same class maps as the C++ path, from the file and from the decoded image."""
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import eig_io
    from top_down_renderer_amd.top_down_map import color_key
    exe = str(tmp_path / "facade_color_png")
    build.build()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_color_png.cpp"), "-o", exe, "-L",
                    os.path.dirname(_lib.SO_PATH), "-ltdr_hip", "-Wl,-rpath," + os.path.dirname(_lib.SO_PATH)], check=True)
    rng = np.random.default_rng(9)
    H, W = 180, 240
    extra = np.array([[255, 255, 255], [1, 2, 3]], np.uint8)         # colours outside the table
    rgb = np.concatenate([np.array(FACADE_RGB, np.uint8), extra])
    coarse = rng.integers(0, len(rgb), (H // 10, W // 10))
    img_rgb = rgb[np.repeat(np.repeat(coarse, 10, 0), 10, 1)]
    png = tmp_path / "site.png"
    png.write_bytes(encode(img_rgb.astype(np.uint32), 2, 8, ftypes=(0, 1, 2, 3, 4), idat_pieces=3))
    (tmp_path / "bad.png").write_bytes(png.read_bytes()[:200])
    (tmp_path / "site.jpg").write_bytes(b"\xff\xd8\xff\xe0 not decoded")
    r = subprocess.run([exe, str(png), str(tmp_path / "cache"), str(tmp_path / "bad.png"), str(tmp_path / "cache_bad"),
                        str(tmp_path / "site.jpg"), str(tmp_path / "cache_jpg")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == sorted(["facade_color_png", "site.png", "bad.png", "site.jpg", "cache"])
    assert not os.path.exists(tmp_path / "site_raster_cache")
    # the Python path, same parameters as the C++ program (facade_color_png.cpp: params())
    p = pkg.Params(flatten_lut=[1, 2, 2, 3, 0, 3], num_classes=4, resolution=1.0)
    keys = [color_key(c[::-1]) for c in FACADE_RGB]
    m = pkg.TopDownMap(p, kernels=kern)
    for src in (str(png), img_rgb[..., ::-1]):
        m.loadColorRasterMap(src, keys)
        assert m.haveMap() and (m.rows, m.cols) == (H, W)
        for c in range(4):
            cm = eig_io.read_eig(str(tmp_path / "cache" / f"class_map{c}.eig"), np.float32)   # [row, col]
            assert np.array_equal(cm.T, m.maps_cm_host[c])
