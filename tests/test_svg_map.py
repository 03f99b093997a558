"""The static vector map (include/tdr.h: tdr_svg_parse_host, tdr_map_load_polygons, tdr_map_load_svg): the host SVG
reader against what the reference's own reader (nanosvg) made of the fixtures (tests/golden/svg_nanosvg.npz, written by
tests/golden/make_svg_golden.py), the reader's defences, the argument checks, and the GPU fill against two independent
NumPy restatements of getClasses (src/top_down_map.cpp:328-365):
  - brute force: every cell against every edge, the reference's expression in f32, product of signs, max over polygons;
  - scanline: per (row, polygon) the crossings' column counts, sorted and paired.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from top_down_renderer_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVG_DIR = os.path.join(ROOT, "tests", "golden", "svg")
GOLDEN = os.path.join(ROOT, "tests", "golden", "svg_nanosvg.npz")
FIXTURES = sorted(f[:-4] for f in os.listdir(SVG_DIR) if f.endswith(".svg"))
vp = C.c_void_p


def lib():
    build.build()
    return _lib.load()


def parse(path):
    from top_down_renderer_amd.kernels import svg_parse
    build.build()
    return svg_parse(path)


# ---- the two restatements ---------------------------------------------------------------------------------------
def sample_tables(W, H, res):
    """samplePts(center = (W, H) / 2, rot 0) of getRasterMap (:391-408), by the oracle: py per row, px per column."""
    from oracle import c_oracle
    c_oracle.build()
    rows, cols = int(np.float32(H) / np.float32(res)), int(np.float32(W) / np.float32(res))
    pts = c_oracle.sample_pts(np.float32(W) / np.float32(2), np.float32(H) / np.float32(2), 0.0, cols, rows, res)
    return pts[:rows, 0].copy(), pts[::rows, 1].copy()


def exclusive_apply(planes, exclusive):
    """getClasses :356-365 literally: plane[u] += 1 - plane[c] for listed u < c, then min(., 1)."""
    planes = planes.astype(np.float32)
    for u in exclusive:
        for c in exclusive:
            if u < c:
                planes[u] += 1 - planes[c]
        planes[u] = np.minimum(planes[u], 1)
    return planes.astype(np.uint8)


def brute_planes(polys, cls, ncls, W, H, res, exclusive):
    """(ncls, rows, cols) 0 inside / 1 elsewhere: getClasses cell by cell, edge by edge, in f32."""
    py, px = sample_tables(W, H, res)
    rows, cols = len(py), len(px)
    fills = -np.ones((ncls, rows, cols), np.float32)
    f32 = np.float32
    with np.errstate(all="ignore"):
        for v, c in zip(polys, cls):
            if not 0 <= c < ncls:
                continue
            buf = -np.ones((rows, cols), np.float32)
            n = len(v)
            j = n - 1
            for i in range(n):
                a, b = v[i], v[j]
                c1 = (py < a[1]) != (py < b[1])
                xc = f32(a[0]) + (f32(b[0] - a[0]) * (py - f32(a[1]))) / f32(b[1] - a[1])
                hit = c1[:, None] & (px[None, :] < xc[:, None])
                buf *= np.where(hit, f32(-1), f32(1))
                j = i
            fills[c] = np.maximum(fills[c], buf)
    planes = ((fills * -1 + 1) / 2).astype(np.uint8)
    return exclusive_apply(planes, exclusive)


def scanline_planes(polys, cls, ncls, W, H, res, exclusive):
    """The same from crossings: per edge its rows, per crossing J = #{j : px_j < xc}, per (row, polygon) the sorted J's
    paired from the top; counts per class, count > 0 inside; exclusive classes as bit masks."""
    py, px = sample_tables(W, H, res)
    rows, cols = len(py), len(px)
    diff = np.zeros((ncls, rows, cols + 1), np.int64)
    keep = [(p, np.asarray(v, np.float32), c) for p, (v, c) in enumerate(zip(polys, cls)) if 0 <= c < ncls and len(v) > 1]
    if keep:
        A, B, P, CL = [], [], [], []
        for p, v, c in keep:
            A.append(v)
            B.append(np.roll(v, 1, axis=0))
            P.append(np.full(len(v), p))
            CL.append(np.full(len(v), c))
        A, B, P, CL = np.concatenate(A), np.concatenate(B), np.concatenate(P), np.concatenate(CL)
        ka = np.searchsorted(py, A[:, 1], "left")
        kb = np.searchsorted(py, B[:, 1], "left")
        ka[np.isnan(A[:, 1])] = 0
        kb[np.isnan(B[:, 1])] = 0
        lo, cnt = np.minimum(ka, kb), np.abs(ka - kb)
        e = np.repeat(np.arange(len(A)), cnt)
        row = lo[e] + (np.arange(len(e)) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        with np.errstate(all="ignore"):
            y = py[row]
            xc = A[e, 0] + ((B[e, 0] - A[e, 0]) * (y - A[e, 1])) / (B[e, 1] - A[e, 1])
        J = np.searchsorted(px, xc, "left")
        J[np.isnan(xc)] = 0
        order = np.lexsort((J, row, P[e]))
        pe, re, Je, ce = P[e][order], row[order], J[order], CL[e][order]
        start = np.r_[True, (pe[1:] != pe[:-1]) | (re[1:] != re[:-1])]
        gid = np.cumsum(start) - 1
        gstart = np.flatnonzero(start)
        gsize = np.diff(np.r_[gstart, len(pe)])
        rank_from_top = gsize[gid] - 1 - (np.arange(len(pe)) - gstart[gid])
        # the k-th from the top (0-based) closes an interval when k is even; it opens at the next one down, or at 0
        closing = np.flatnonzero(rank_from_top % 2 == 0)
        opens = np.where(rank_from_top[closing] + 1 < gsize[gid[closing]], Je[np.maximum(closing - 1, 0)], 0)
        ends = Je[closing]
        ok = opens < ends
        np.add.at(diff, (ce[closing][ok], re[closing][ok], opens[ok]), 1)
        np.add.at(diff, (ce[closing][ok], re[closing][ok], ends[ok]), -1)
    inside = np.cumsum(diff, axis=2)[:, :, :cols] > 0
    listed = set(int(x) for x in exclusive)
    out = inside.copy()
    for u in listed:
        for c in listed:
            if c > u:
                out[u] &= ~inside[c]
    return np.where(out, 0, 1).astype(np.uint8)


def random_case(rng, W, H, n_poly, ncls, py=None, px=None):
    polys, cls = [], []
    for _ in range(n_poly):
        kind = rng.integers(0, 7)
        n = int(rng.integers(3, 9))
        cx, cy = rng.uniform(-0.2 * W, 1.2 * W), rng.uniform(-0.2 * H, 1.2 * H)
        r = rng.uniform(0.05, 0.6) * max(W, H)
        v = np.stack([cx + r * rng.uniform(-1, 1, n), cy + r * rng.uniform(-1, 1, n)], 1).astype(np.float32)
        if kind == 0 and py is not None:        # vertices exactly on sample coordinates
            v[:, 1] = rng.choice(py, n)
            v[:, 0] = rng.choice(px, n)
        elif kind == 1:                         # axis-aligned: horizontal and vertical edges
            x0, x1, y0, y1 = np.float32(np.sort(rng.uniform(0, W, 2))).tolist() + np.float32(np.sort(rng.uniform(0, H, 2))).tolist()
            v = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float32)
        elif kind == 2:                         # duplicate vertices
            v = np.repeat(v, 2, axis=0)
        elif kind == 3:                         # 1 or 2 vertices
            v = v[: int(rng.integers(1, 3))]
        elif kind == 4:                         # wholly off the map
            v[:, 0] += np.float32(3 * W)
        # (kind 5, 6: random, usually self-intersecting)
        polys.append(v)
        cls.append(int(rng.integers(-1, ncls + 1)) if rng.random() < 0.1 else int(rng.integers(0, ncls)))
    return polys, cls


# ---- CPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_parser_matches_nanosvg(name):
    g = np.load(GOLDEN)
    size, keys, offs, verts = parse(os.path.join(SVG_DIR, name + ".svg"))
    assert size.tobytes() == g[f"{name}/size"].tobytes()

    def polys(k, o, v):
        return sorted(((int(k[p]), v[o[p]:o[p + 1]]) for p in range(len(k))),
                      key=lambda t: (t[0], len(t[1]), np.round(t[1].astype(np.float64), 2).tobytes()))
    mine, ref = polys(keys, offs, verts), polys(g[f"{name}/keys"], g[f"{name}/offs"], g[f"{name}/verts"])
    assert [(k, len(v)) for k, v in mine] == [(k, len(v)) for k, v in ref]
    for (ka, va), (kb, vb) in zip(mine, ref):
        if name == "arcs":   # the arc's split points come from cosf / sinf: 4 ulp allowed, the counts are exact
            ulp = np.abs(va.view(np.int32).astype(np.int64) - vb.view(np.int32).astype(np.int64))
            assert ulp.max() <= 4
        else:
            assert va.tobytes() == vb.tobytes()


def test_fill_keys_and_quirks():
    """The fill-key rules: #rgb / rgb() / keywords stored 0xBBGGRR, none and absent fill -> 0, an unknown keyword ->
    grey, a gradient -> no key, an unresolved gradient -> 0; an open subpath loses its last vertex."""
    from top_down_renderer_amd.top_down_map import parse_svg, svg_fill_key
    (w, h), polys = parse_svg(os.path.join(SVG_DIR, "shapes.svg"))
    assert (w, h) == (240.0, 180.0)
    keys = [k for k, _ in polys]
    assert keys[0] == keys[1] == 0x0000FF == svg_fill_key((0, 0, 255))     # #ff0000, #f00
    assert 0x808080 in keys and 0 in keys
    open_path = [v for k, v in polys if k == 0x0000FF and len(v) == 2]
    assert any(np.array_equal(v, np.array([[60, 180 - 60], [70, 180 - 60]], np.float32)) for v in open_path)
    (_, _), gp = parse_svg(os.path.join(SVG_DIR, "defs_gradient.svg"))
    assert [k for k, _ in gp][:3] == [None, None, 0]


def test_parser_is_defensive(tmp_path):
    """Truncations, byte flips and hand-made bad files: TDR_OK or a TDR_ERR_* with a message, never a crash."""
    L = lib()
    size = np.zeros(2, np.float32)

    def run(data):
        p = tmp_path / "f.svg"
        p.write_bytes(data)
        n_p, n_v = C.c_int64(0), C.c_int64(0)
        rc = L.tdr_svg_parse_host(str(p).encode(), size.ctypes.data_as(vp), C.byref(n_p), C.byref(n_v), None, None, None)
        assert rc in (0, -1, -3), rc
        if rc == 0 and n_p.value < 100000 and n_v.value < 1000000:
            k = np.zeros(n_p.value + 1, np.uint32)
            o = np.zeros(n_p.value + 1, np.int64)
            v = np.zeros((n_v.value + 1, 2), np.float32)
            assert L.tdr_svg_parse_host(str(p).encode(), size.ctypes.data_as(vp), C.byref(n_p), C.byref(n_v),
                                        k.ctypes.data_as(vp), o.ctypes.data_as(vp), v.ctypes.data_as(vp)) == 0
            assert o[0] == 0 and np.all(np.diff(o[:n_p.value + 1]) >= 0) and np.isfinite(v).all()
        else:
            assert rc == 0 or L.tdr_last_error()
        return rc
    rng = np.random.default_rng(5)
    for name in ("shapes", "arcs"):
        src = open(os.path.join(SVG_DIR, name + ".svg"), "rb").read()
        for n in range(len(src) + 1):
            run(src[:n])
        for _ in range(100):
            b = bytearray(src)
            for _ in range(int(rng.integers(1, 6))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            run(bytes(b))
    bad = [b"", b"<svg>", b"<svg width='10'>", b"<svg width='-5' height='5'/>", b"<svg width='1e999' height='10'>",
           b"<svg width='10' height='10'><path d='M1e39 0 L1 1 L2 2 Z'/></svg>",
           b"<svg width='10' height='10'><path d='M0 0 A1e30 1e30 0 1 1 5 5 Z'/></svg>",
           b"<svg width='10' height='10'><path d='M" + b"9" * 5000 + b" 0 L1 1 2 2z'/></svg>",
           b"<svg width='10' height='10'>" + b"<g transform='scale(2)'>" * 400 + b"<rect width='1' height='1'/>",
           b"<svg width='10' height='10'><polygon points='" + b"1,2 " * 20000 + b"'/></svg>",
           b"<svg viewBox='0 0'><rect width='1' height='1'/></svg>", b"<svg width='10\x00' height='10'>",
           b"<svg width='10' height='10'><path d='C1 2 3 4 5 6 L 1 1 Z' fill='rgb(" + b"%" * 100 + b")'/></svg>",
           b"<svg width='10' height='10'><path fill='#12345' d='M 0 0 h 1 v 1 Z' transform='rotate(1 2 3 4 5)'/>",
           b"<" * 1000, b">" * 1000, b"<svg " + b"a='1' " * 300 + b"width='4' height='4'>"]
    for data in bad:
        run(data)
    assert run(b"<svg>") == -1 and b"size" in L.tdr_last_error()
    n_p, n_v = C.c_int64(0), C.c_int64(0)
    assert L.tdr_svg_parse_host(str(tmp_path / "missing.svg").encode(), size.ctypes.data_as(vp), C.byref(n_p),
                                C.byref(n_v), None, None, None) == -1


def test_abi_validation():
    """Every argument is checked before any device work (the map handle is checked last: NULL here, no GPU needed)."""
    L = lib()
    v = np.zeros((4, 2), np.float32)
    o = np.array([0, 4], np.int64)
    c = np.zeros(1, np.int32)
    ex_ok = np.array([0, 0, 1], np.int32)
    P = lambda a: a.ctypes.data_as(vp)

    def lp(verts=P(v), offs=P(o), cls=P(c), n=1, W=10, H=10, ncls=3, ex=P(ex_ok), nex=3, res=1.0):
        rc = L.tdr_map_load_polygons(None, verts, offs, cls, n, W, H, ncls, ex, nex, C.c_float(res), 0, 0, None)
        return rc, L.tdr_last_error().decode()
    assert lp()[0] == -1 and "null map" in lp()[1]
    for kw, msg in ((dict(verts=None), "null polygon"), (dict(offs=None), "null polygon"), (dict(cls=None), "null polygon"),
                    (dict(n=-1), "null polygon"), (dict(ncls=0), "num_classes"), (dict(ncls=16), "num_classes"),
                    (dict(ex=P(np.array([0, 3], np.int32)), nex=2), "exclusive"),
                    (dict(ex=P(np.array([-1], np.int32)), nex=1), "exclusive"), (dict(ex=None, nex=2), "exclusive"),
                    (dict(res=0.0), "resolution"), (dict(res=-1.0), "resolution"), (dict(res=float("nan")), "resolution"),
                    (dict(res=0.1), "resolution"), (dict(W=0), "size"), (dict(H=-3), "size"),
                    (dict(offs=P(np.array([0, -1], np.int64))), "offsets")):
        rc, err = lp(**kw)
        assert rc == -1 and msg in err, (kw, err)
    out = np.zeros(300, np.uint8)

    def pp(verts=P(v), offs=P(o), cls=P(c), n=1, W=10, H=10, ncls=3, ex=P(ex_ok), nex=3, res=1.0, planes=P(out)):
        rc = L.tdr_polygon_planes(verts, offs, cls, n, W, H, ncls, ex, nex, C.c_float(res), planes)
        return rc, L.tdr_last_error().decode()
    for kw, msg in ((dict(verts=None), "null polygon"), (dict(ncls=16), "num_classes"), (dict(res=0.0), "resolution"),
                    (dict(ex=P(np.array([3], np.int32)), nex=1), "exclusive"), (dict(W=0), "size"),
                    (dict(offs=P(np.array([0, -1], np.int64))), "offsets"), (dict(planes=None), "planes_out")):
        rc, err = pp(**kw)
        assert rc == -1 and msg in err, (kw, err)
    keys = np.zeros(2, np.uint32)
    lut = np.zeros(2, np.int32)

    def ls(path=b"x.svg", keys_=P(keys), lut_=P(lut), n=2, ncls=3, ex=P(ex_ok), nex=3, res=1.0):
        rc = L.tdr_map_load_svg(None, path, keys_, lut_, n, ncls, ex, nex, C.c_float(res), 0, 0)
        return rc, L.tdr_last_error().decode()
    assert ls()[0] == -1 and "null map" in ls()[1]
    for kw, msg in ((dict(path=None), "null path"), (dict(keys_=None), "null path"), (dict(lut_=None), "null path"),
                    (dict(ncls=0), "num_classes"), (dict(ex=P(np.array([5], np.int32)), nex=1), "exclusive"),
                    (dict(res=0.0), "resolution")):
        rc, err = ls(**kw)
        assert rc == -1 and msg in err, (kw, err)
    size = np.zeros(2, np.float32)
    n_p, n_v = C.c_int64(0), C.c_int64(0)
    f = os.path.join(SVG_DIR, "shapes.svg").encode()
    assert L.tdr_svg_parse_host(None, P(size), C.byref(n_p), C.byref(n_v), None, None, None) == -1
    assert L.tdr_svg_parse_host(f, None, C.byref(n_p), C.byref(n_v), None, None, None) == -1
    assert L.tdr_svg_parse_host(f, P(size), C.byref(n_p), C.byref(n_v), None, None, None) == 0 and n_p.value == 24
    k, oo, vv = np.zeros(24, np.uint32), np.zeros(25, np.int64), np.zeros((10, 2), np.float32)
    n_v.value = 10                                                                                   # capacities
    assert L.tdr_svg_parse_host(f, P(size), C.byref(n_p), C.byref(n_v), P(k), P(oo), P(vv)) == -1   # too small
    assert L.tdr_svg_parse_host(f, P(size), C.byref(n_p), C.byref(n_v), P(k), None, P(vv)) == -1


@pytest.mark.parametrize("seed", range(6))
def test_restatements_agree(seed):
    rng = np.random.default_rng(100 + seed)
    W, H, res = [(17, 13, 1.0), (30, 9, 0.5), (40, 41, 2.5), (1, 20, 1.0), (25, 1, 1.0), (12, 12, 1.0)][seed]
    ncls = 4
    py, px = sample_tables(W, H, res)
    polys, cls = random_case(rng, W, H, 12, ncls, py, px)
    excl = [0] * ncls + [2, 3, 1]
    a = brute_planes(polys, cls, ncls, W, H, res, excl)
    b = scanline_planes(polys, cls, ncls, W, H, res, excl)
    assert np.array_equal(a, b)
    assert (a == 0).any() and (a == 1).any()


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


def flat(polys):
    verts = np.concatenate([np.asarray(v, np.float32).reshape(-1, 2) for v in polys]) if polys else np.zeros((0, 2), np.float32)
    offs = np.r_[0, np.cumsum([len(v) for v in polys])].astype(np.int64)
    return verts, offs


SHAPES = [(1, 63, 1.0), (63, 65, 1.0), (65, 257, 1.0), (257, 1, 1.0), (63, 1, 1.0), (32, 33, 0.5), (128, 32, 0.5),
          (160, 163, 2.5), (642, 3, 2.5), (5, 160, 2.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(30))
def test_gpu_fill_matches_bruteforce(kern, handle, case):
    rng = np.random.default_rng(1000 + case)
    H, W, res = SHAPES[case % len(SHAPES)]
    ncls = int(rng.integers(1, 7))
    py, px = sample_tables(W, H, res)
    polys, cls = random_case(rng, W, H, int(rng.integers(1, 14)), ncls, py, px)
    excl = [0] * ncls + sorted(set(int(x) for x in rng.integers(0, ncls, 3)))     # the node's list (top_down_render.cpp:177-181)
    verts, offs = flat(polys)
    planes = kern.map_load_polygons(handle, verts, offs, np.asarray(cls, np.int32), W, H, ncls, excl, res)
    want = brute_planes(polys, cls, ncls, W, H, res, excl)
    assert planes.shape == (ncls, len(px), len(py))
    assert np.array_equal(np.transpose(planes, (0, 2, 1)), want)
    alone = kern.polygon_planes(verts, offs, np.asarray(cls, np.int32), W, H, ncls, excl, res)   # the fill-only entry
    assert np.array_equal(alone, planes)


def synthetic_city(rng, size=4000, n_poly=10000, ncls=6):
    """~10 000 polygons over 6 classes: roads as long thin quads, blocks, buildings with many vertices, a few big
    regions spanning the map (the load the timing tool measures too)."""
    polys, cls = [], []
    for _ in range(n_poly):
        kind = rng.random()
        if kind < 0.2:                          # road: long thin quad
            x0, y0 = rng.uniform(0, size, 2)
            ang = rng.uniform(0, np.pi)
            L, wd = rng.uniform(200, 2000), rng.uniform(4, 20)
            d, nrm = np.array([np.cos(ang), np.sin(ang)]), np.array([-np.sin(ang), np.cos(ang)])
            p0 = np.array([x0, y0])
            v = np.stack([p0, p0 + L * d, p0 + L * d + wd * nrm, p0 + wd * nrm])
            c = 1
        elif kind < 0.995:                      # building / block: star-shaped polygon
            n = int(rng.integers(4, 24))
            cx, cy = rng.uniform(0, size, 2)
            r = rng.uniform(5, 60) * rng.uniform(0.6, 1.0, n)
            t = np.sort(rng.uniform(0, 2 * np.pi, n))
            v = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)
            c = int(rng.integers(2, ncls))
        else:                                   # large region
            n = int(rng.integers(20, 200))
            cx, cy = rng.uniform(0, size, 2)
            r = rng.uniform(500, 2500) * rng.uniform(0.5, 1.0, n)
            t = np.sort(rng.uniform(0, 2 * np.pi, n))
            v = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)
            c = 0
        polys.append(v.astype(np.float32))
        cls.append(c)
    return polys, cls


@pytest.mark.gpu
def test_gpu_fill_full_size(kern, handle, tmp_path):
    """4000 x 4000 px, 10 000 polygons: the planes equal the scanline restatement, and the map the handle holds (class
    maps, mask, geometric layers: the .eig cache files) is byte for byte the map tdr_map_load_rasters builds from the same
    planes written as class<i>.png."""
    from top_down_renderer_amd._lib import check
    rng = np.random.default_rng(4000)
    polys, cls = synthetic_city(rng)
    ncls, W, H, res = 6, 4000, 4000, 1.0
    excl = [0] * ncls + [1, 5]
    verts, offs = flat(polys)
    planes = kern.map_load_polygons(handle, verts, offs, np.asarray(cls, np.int32), W, H, ncls, excl, res)
    want = scanline_planes(polys, cls, ncls, W, H, res, excl)
    assert np.array_equal(np.transpose(planes, (0, 2, 1)), want)
    d = tmp_path / "rasters"
    d.mkdir()
    for c in range(ncls):
        kern.png_write_gray8(str(d / f"class{c}.png"), np.where(planes[c].T == 0, 0, 255).astype(np.uint8)[::-1])
    m2 = vp()
    check(kern.lib.tdr_map_create(C.byref(m2)))
    try:
        check(kern.lib.tdr_map_load_rasters(m2, str(d).encode(), ncls, C.c_float(res), 0, 0))
        for m, sub in ((handle, "a"), (m2, "b")):
            check(kern.lib.tdr_map_save_cache(m, str(tmp_path / sub).encode(), b"city.svg"))
        for f in sorted(os.listdir(tmp_path / "a")):
            assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
        assert len(os.listdir(tmp_path / "a")) == ncls + 4   # cached_data.txt, class maps, mask, two geo layers
    finally:
        kern.lib.tdr_map_destroy(m2)


LUT_KEYS = [0x0000FF, 0x008000, 0x00FF00, 0xFF0000, 0x000000, 0x808080, 0xFFFF00, 0x0000FF]
LUT_FLAT = [1, 2, 2, 3, 0, 3, 7, 2]          # the 7 is outside [0, 4): skipped like the reference's undefined case


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_gpu_svg_end_to_end_against_nanosvg_polygons(kern, handle, tmp_path, name):
    """tdr_map_load_svg on a fixture gives the planes the restatement gives from the polygons nanosvg produced."""
    from top_down_renderer_amd._lib import check
    g = np.load(GOLDEN)
    size, keys, offs, verts = g[f"{name}/size"], g[f"{name}/keys"], g[f"{name}/offs"], g[f"{name}/verts"]
    ncls, res = 4, (0.5 if name == "arcs" else 1.0)
    excl = [0] * ncls + [2, 3]
    polys, cls = [], []
    for lut_i, fl in enumerate(LUT_FLAT):    # loadSvg :77-103
        if not 0 <= fl < ncls:
            continue
        for p in range(len(keys)):
            if int(keys[p]) == LUT_KEYS[lut_i]:
                polys.append(verts[offs[p]:offs[p + 1]])
                cls.append(fl)
    W, H = int(size[0]), int(size[1])
    want = brute_planes(polys, cls, ncls, W, H, res, excl)
    kern.map_load_svg(handle, os.path.join(SVG_DIR, name + ".svg"), LUT_KEYS, LUT_FLAT, ncls, excl, res)
    check(kern.lib.tdr_map_save_rasters(handle, str(tmp_path / "r").encode()))
    got = np.stack([kern.png_read_gray8(str(tmp_path / "r" / f"class{c}.png"))[::-1] for c in range(ncls)])
    assert np.array_equal(np.where(got == 0, 0, 1), want)


@pytest.mark.gpu
def test_facade_svg_constructor_and_python_path(kern, tmp_path):
    """tests/cpp/facade_svg.cpp: TopDownMap(params) with a .svg map_path — parse, fill, raster cache, distance maps,
    map cache; the second construction hits the cache; a bad SVG leaves the map empty and writes nothing.  The Python
    loadVectorMap builds the same class maps as the C++ path."""
    import shutil
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import eig_io
    exe = str(tmp_path / "facade_svg")
    build.build()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_svg.cpp"), "-o", exe, "-L", os.path.dirname(_lib.SO_PATH),
                    "-ltdr_hip", "-Wl,-rpath," + os.path.dirname(_lib.SO_PATH)], check=True)
    svg = tmp_path / "site.svg"
    shutil.copy(os.path.join(SVG_DIR, "shapes.svg"), svg)
    (tmp_path / "bad.svg").write_text("<svg><rect width='3' height='3'/></svg>")
    r = subprocess.run([exe, str(svg), str(tmp_path / "cache"), str(tmp_path / "bad.svg"), str(tmp_path / "cache_bad")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.isdir(tmp_path / "site_raster_cache")
    assert sorted(os.listdir(tmp_path / "site_raster_cache")) == [f"class{c}.png" for c in range(4)]
    assert not os.path.exists(tmp_path / "bad_raster_cache") and not os.path.exists(tmp_path / "cache_bad")
    # the Python path: same parameters as the C++ program
    p = pkg.Params(flatten_lut=[1, 2, 2, 3, 0, 3], num_classes=4, exclusive_classes=[0, 0, 0, 0, 2, 3], resolution=1.0)
    m = pkg.TopDownMap(p, kernels=kern)
    m.loadVectorMap(str(svg), LUT_KEYS[:6])
    assert m.haveMap()
    for c in range(4):
        cm = eig_io.read_eig(str(tmp_path / "cache" / f"class_map{c}.eig"), np.float32)   # [row, col]
        assert np.array_equal(cm.T, m.maps_cm_host[c])
