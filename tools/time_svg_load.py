"""Times the static vector map's load (include/tdr.h) in three parts: parse (tdr_svg_parse_host, host), fill
(tdr_polygon_planes: getRasterMap + getClasses on the GPU) and ingest (geometric layers + exact distance transforms,
the raster cache's device path), and the handle call that does fill and ingest together (tdr_map_load_polygons).
Map: a synthetic 4000 x 4000 px SVG with ~10 000 polygons over 6 classes (roads, blocks, buildings, a few large regions) and the node's exclusive list ([0] * 6 + [1, 5]).  Also times the tests' NumPy
scanline restatement of getClasses on a REDUCED map (1000 x 1000 px, 1/16 of the polygons), labelled as such.

    python tools/time_svg_load.py [--reps 5] [--out profiles/<name>.txt]
Prints one JSON line; --out also writes it (with the device name) to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLORS = ["#808080", "#ffffff", "#ff0000", "#00ff00", "#0000ff", "#ffff00"]   # class c <- COLORS[c]


def synthetic_svg(path, size=4000, n_poly=10000, seed=0):
    rng = np.random.default_rng(seed)
    out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{size}" height="{size}">']
    for _ in range(n_poly):
        kind = rng.random()
        if kind < 0.2:
            x0, y0 = rng.uniform(0, size, 2)
            ang = rng.uniform(0, np.pi)
            L, wd = rng.uniform(200, 2000), rng.uniform(4, 20)
            d, nrm = np.array([np.cos(ang), np.sin(ang)]), np.array([-np.sin(ang), np.cos(ang)])
            p0 = np.array([x0, y0])
            v, c = np.stack([p0, p0 + L * d, p0 + L * d + wd * nrm, p0 + wd * nrm]), 1
        elif kind < 0.995:
            n = int(rng.integers(4, 24))
            cx, cy = rng.uniform(0, size, 2)
            r = rng.uniform(5, 60) * rng.uniform(0.6, 1.0, n)
            t = np.sort(rng.uniform(0, 2 * np.pi, n))
            v, c = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1), int(rng.integers(2, 6))
        else:
            n = int(rng.integers(20, 200))
            cx, cy = rng.uniform(0, size, 2)
            r = rng.uniform(500, 2500) * rng.uniform(0.5, 1.0, n)
            t = np.sort(rng.uniform(0, 2 * np.pi, n))
            v, c = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1), 0
        d = "M" + " L".join(f"{x:.2f} {y:.2f}" for x, y in v) + " Z"
        out.append(f'<path d="{d}" fill="{COLORS[c]}"/>')
    out.append("</svg>")
    open(path, "w").write("\n".join(out))


def keys_and_lut():
    from top_down_renderer_amd.top_down_map import svg_fill_key
    keys = []
    for c in COLORS:   # nanosvg's 0xBBGGRR of #RRGGBB = svg_fill_key((b, g, r))
        r, g, b = int(c[1:3], 16), int(c[3:5], 16), int(c[5:7], 16)
        keys.append(svg_fill_key((b, g, r)))
    return keys, list(range(len(COLORS)))


def assign(polys, keys, lut, ncls):
    verts, offs, cls = [], [0], []
    for i, fl in enumerate(lut):
        if 0 <= fl < ncls:
            for k, v in polys:
                if k == keys[i]:
                    verts.append(v)
                    offs.append(offs[-1] + len(v))
                    cls.append(fl)
    return np.concatenate(verts), np.asarray(offs, np.int64), np.asarray(cls, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from top_down_renderer_amd import build
    from top_down_renderer_amd._lib import check
    from top_down_renderer_amd.kernels import HipKernels
    from top_down_renderer_amd.top_down_map import parse_svg
    build.build()
    k = HipKernels()
    ncls, res, excl = 6, 1.0, [0] * 6 + [1, 5]
    keys, lut = keys_and_lut()
    tmp = tempfile.mkdtemp(prefix="tdr_svg_time_")
    path = os.path.join(tmp, "city.svg")
    synthetic_svg(path)
    med = lambda xs: float(np.median(xs))

    (w, h), polys = parse_svg(path)
    lib = k.lib
    size = np.zeros(2, np.float32)
    t_parse = []
    for _ in range(args.reps + 1):   # one parse: the size query of tdr_svg_parse_host
        n_p, n_v = C.c_int64(0), C.c_int64(0)
        t0 = time.perf_counter()
        check(lib.tdr_svg_parse_host(path.encode(), size.ctypes.data_as(C.c_void_p), C.byref(n_p), C.byref(n_v),
                                     None, None, None))
        t_parse.append(time.perf_counter() - t0)
    verts, offs, cls = assign(polys, keys, lut, ncls)
    m = C.c_void_p()
    check(lib.tdr_map_create(C.byref(m)))
    t_fill, t_ingest, t_total = [], [], []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()   # the fill alone: host plan, device buffers, kernels, planes back to the host
        planes = k.polygon_planes(verts, offs, cls, int(w), int(h), ncls, excl, res)
        t_fill.append(time.perf_counter() - t0)
        raster = np.ascontiguousarray(np.where(np.transpose(planes, (0, 2, 1)) == 0, 0, 255).astype(np.uint8)[:, ::-1])
        torch.cuda.synchronize()
        t0 = time.perf_counter()   # the ingest alone: planes up, geometric layers + distance transforms, compact records
        dev = k.make_map_from_rasters(raster, res)
        torch.cuda.synchronize()
        t_ingest.append(time.perf_counter() - t0)
        del dev
        t0 = time.perf_counter()   # both in one handle call (its ingest also keeps host copies of the class maps)
        k.map_load_polygons(m, verts, offs, cls, int(w), int(h), ncls, excl, res, want_planes=False)
        torch.cuda.synchronize()
        t_total.append(time.perf_counter() - t0)
    lib.tdr_map_destroy(m)
    n_poly, n_vert = len(cls), len(verts)
    # the NumPy restatement on a reduced map
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_svg_map import scanline_planes
    small = os.path.join(tmp, "small.svg")
    synthetic_svg(small, size=1000, n_poly=625, seed=1)
    (ws, hs), ps = parse_svg(small)
    sv, so, sc = assign(ps, keys, lut, ncls)
    sp = [sv[so[i]:so[i + 1]] for i in range(len(sc))]
    t0 = time.perf_counter()
    scanline_planes(sp, list(sc), ncls, int(ws), int(hs), res, excl)
    t_np = time.perf_counter() - t0
    rec = {"map_px": [int(w), int(h)], "cells": [planes.shape[2], planes.shape[1]], "classes": ncls,
           "polygons": int(n_poly), "vertices": int(n_vert), "reps": args.reps,
           "parse_ms": round(1e3 * med(t_parse[1:]), 2),
           "fill_ms": round(1e3 * med(t_fill[1:]), 2),
           "ingest_ms": round(1e3 * med(t_ingest[1:]), 2),
           "load_polygons_ms": round(1e3 * med(t_total[1:]), 2),
           "numpy_scanline_reduced_1000px_625poly_ms": round(1e3 * t_np, 1),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(
            "# tools/time_svg_load.py: static vector map load, median of --reps after one warm-up, wall clock.\n"
            "# parse_ms: one tdr_svg_parse_host size query (one parse).  fill_ms: tdr_polygon_planes (host plan, device\n"
            "# buffers, fill kernels, planes read back).  ingest_ms: the raster ingest of those planes (upload, geometric layers,\n"
            "# distance transforms, compact records).  load_polygons_ms: tdr_map_load_polygons, fill + ingest + host copies.\n"
            "# The NumPy figure is the tests' restatement on a REDUCED map.\n"
            + line + "\n")


if __name__ == "__main__":
    main()
