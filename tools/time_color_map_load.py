"""Times the static colour raster map's load (include/tdr.h) in parts: read (tdr_png_read_color_host: inflate, unfilter,
conversion to BGR, host), upload (the BGR image to the device), the colour ingest on the device (tdr_k_map_from_color:
the colour lookup per cell + the exact distance transforms), the same distance transforms behind a label image
(tdr_k_map_from_labels on the colour map's color2Ind image: a one-byte gather instead of the lookup), the whole-image
lookup alone (tdr_k_color_index), and the handle call that does everything (tdr_map_load_color_png: read, upload, ingest,
host copies, compact records).  Device parts are timed with events on the stream; read and the handle call by the wall
clock.
Map: a synthetic 4000 x 4000 RGB PNG (8-bit, colour type 2) of 6 class colours in blocks, roads and noise, plus 2 % of
pixels in colours outside the table; zlib's default level, each row's filter chosen like libpng's adaptive heuristic
(least sum of absolute filtered bytes).

    python tools/time_color_map_load.py [--reps 5] [--out profiles/<name>.txt]
Prints one JSON line; --out also writes it (with the device name) to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RGB = [(128, 128, 128), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0)]   # class c <- RGB[c]


def synthetic_rgb(size=4000, seed=0):
    rng = np.random.default_rng(seed)
    cls = np.repeat(np.repeat(rng.integers(2, 6, (size // 40, size // 40)), 40, 0), 40, 1)   # blocks
    cls[rng.random((size, size)) < 0.02] = 0
    for _ in range(60):                                                                     # roads
        if rng.random() < 0.5:
            y, w = int(rng.integers(0, size - 20)), int(rng.integers(4, 20))
            cls[y:y + w] = 1
        else:
            x, w = int(rng.integers(0, size - 20)), int(rng.integers(4, 20))
            cls[:, x:x + w] = 1
    img = np.asarray(RGB, np.uint8)[cls]
    stray = rng.random((size, size)) < 0.02                                                 # unmatched colours
    img[stray] = rng.integers(0, 256, (int(stray.sum()), 3)).astype(np.uint8) | np.uint8(1)
    return img


def write_png(path, rgb):
    """8-bit RGB PNG, adaptive filters (per row the filter with the least sum of |signed filtered byte|), level 6."""
    h, w, _ = rgb.shape
    r = rgb.reshape(h, w * 3).astype(np.int16)
    up = np.vstack([np.zeros((1, w * 3), np.int16), r[:-1]])
    left = np.hstack([np.zeros((h, 3), np.int16), r[:, :-3]])
    ul = np.hstack([np.zeros((h, 3), np.int16), up[:, :-3]])
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cand = np.stack([r, r - left, r - up, r - ((left + up) >> 1), r - paeth]) & 0xFF
    score = np.where(cand < 128, cand, 256 - cand).sum(axis=2)
    ft = score.argmin(axis=0)
    rows = np.empty((h, w * 3 + 1), np.uint8)
    rows[:, 0] = ft
    rows[:, 1:] = cand[ft, np.arange(h)].astype(np.uint8)
    z = zlib.compress(rows.tobytes(), 6)

    def chunk(t, d):
        return len(d).to_bytes(4, "big") + t + d + (zlib.crc32(t + d) & 0xFFFFFFFF).to_bytes(4, "big")
    hdr = w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])
    idat = b"".join(chunk(b"IDAT", z[i:i + (1 << 16)]) for i in range(0, len(z), 1 << 16))   # 64 KiB chunks
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", hdr) + idat + chunk(b"IEND", b""))
    return len(z), np.bincount(ft, minlength=5).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from top_down_renderer_amd import build
    from top_down_renderer_amd._lib import check
    from top_down_renderer_amd.kernels import HipKernels, _ptr
    from top_down_renderer_amd.top_down_map import color_key
    build.build()
    k = HipKernels()
    lib = k.lib
    ncls, res = 6, 1.0
    keys = np.array([color_key(c[::-1]) for c in RGB], np.uint32)
    lut = np.arange(ncls, dtype=np.int32)
    tmp = tempfile.mkdtemp(prefix="tdr_color_time_")
    path = os.path.join(tmp, "city.png")
    rgb = synthetic_rgb()
    _, filters = write_png(path, rgb)
    H, W = rgb.shape[:2]
    med = lambda xs: float(np.median(xs))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    bgr = np.empty((H, W, 3), np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    t_read = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        check(lib.tdr_png_read_color_host(path.encode(), vp(bgr), bgr.size, C.byref(w), C.byref(h)))
        t_read.append(time.perf_counter() - t0)
    assert np.array_equal(bgr, rgb[..., ::-1])
    dev = torch.empty(bgr.size, dtype=torch.uint8, device=k.device)
    host = torch.from_numpy(bgr.reshape(-1))
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    t_up = [timed(lambda: dev.copy_(host)) for _ in range(args.reps + 1)]
    rec = k.empty((int(lib.tdr_map_rec_floats_total(ncls, H, W)),))
    ws = k.empty((int(lib.tdr_map_ingest_workspace_bytes(ncls, H, W)),), torch.uint8)
    idx = k.empty((H, W), torch.uint8)
    st = k.stream()
    t_ingest = [timed(lambda: check(lib.tdr_k_map_from_color(_ptr(dev), H, W, vp(keys), vp(lut), ncls, ncls,
                                                              C.c_float(res), _ptr(rec), _ptr(ws), st)))
                for _ in range(args.reps + 1)]
    t_index = [timed(lambda: check(lib.tdr_k_color_index(_ptr(dev), H, W, vp(keys), ncls, _ptr(idx), st)))
               for _ in range(args.reps + 1)]
    lut_d = k.to_device(lut)
    t_labels = [timed(lambda: check(lib.tdr_k_map_from_labels(_ptr(idx), H, W, _ptr(lut_d), ncls, ncls, C.c_float(res),
                                                               _ptr(rec), _ptr(ws), st)))
                for _ in range(args.reps + 1)]
    del rec, ws, idx, dev
    m = C.c_void_p()
    check(lib.tdr_map_create(C.byref(m)))
    t_total = []
    for _ in range(args.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        check(lib.tdr_map_load_color_png(m, path.encode(), vp(keys), vp(lut), ncls, ncls, C.c_float(res), 0, 0))
        t_total.append(time.perf_counter() - t0)
    lib.tdr_map_destroy(m)
    png_bytes = os.path.getsize(path)
    os.remove(path)
    os.rmdir(tmp)
    rec = {"map_px": [W, H], "classes": ncls, "png_bytes": png_bytes,
           "row_filters_none_sub_up_avg_paeth": filters, "reps": args.reps,
           "read_ms": round(1e3 * med(t_read[1:]), 2),
           "upload_ms": round(med(t_up[1:]), 2),
           "map_from_color_ms": round(med(t_ingest[1:]), 2),
           "map_from_labels_ms": round(med(t_labels[1:]), 2),
           "color_index_ms": round(med(t_index[1:]), 3),
           "load_color_png_ms": round(1e3 * med(t_total[1:]), 2),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(
            "# tools/time_color_map_load.py: static colour map load, median of --reps after one warm-up.\n"
            "# read_ms: tdr_png_read_color_host (host: inflate, unfilter, BGR; wall clock).  upload_ms: the BGR image to the\n"
            "# device (events).  map_from_color_ms: tdr_k_map_from_color (events: colour lookup per cell + distance transforms).\n"
            "# map_from_labels_ms: the same distance transforms behind a label image (tdr_k_map_from_labels).  color_index_ms:\n"
            "# tdr_k_color_index over the whole image (events).  load_color_png_ms: tdr_map_load_color_png (wall clock: read,\n"
            "# upload, ingest, host copies of the class maps, compact records).\n"
            + line + "\n")


if __name__ == "__main__":
    main()
