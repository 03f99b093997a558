#!/usr/bin/env python3
"""Times the incremental map update (tdr_map_update_labels_incremental / tdr_map_patch_labels, csrc/tdr_map_incr.hip)
against the full one (tdr_map_set_labels) on a 4000 x 4000 six-class label map, and splits the full path into its stages
(upload, ingest, host copies, compaction, road scan) — the stages are run one by one through the kernel-level ABI.
Device stages are timed with events, calls with the wall clock; medians of `reps`.
    python3 tools/time_map_update_incremental.py [size] [reps]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from top_down_renderer_amd import synth  # noqa: E402
from top_down_renderer_amd._lib import check  # noqa: E402
from top_down_renderer_amd.kernels import DeviceMap, HipKernels, _ptr  # noqa: E402


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ncls, res = 6, 1.0
    k = HipKernels()
    L, vp = k.lib, C.c_void_p
    rng = np.random.default_rng(3)
    lab = synth.make_label_image(size, ncls, rng)
    img = np.where(lab < 0, 255, lab).astype(np.uint8)[::-1].copy()
    lut = np.full(256, -1, np.int32)
    lut[:ncls] = np.arange(ncls)
    print(f"map {size} x {size}, {ncls} classes, resolution {res}; medians of {reps}")

    # ---- the full path, stage by stage ----
    rows = cols = size
    img_d = torch.empty(img.size, dtype=torch.uint8, device=k.device)
    img_pin = torch.from_numpy(img.reshape(-1)).pin_memory()
    lut_d = k.to_device(lut)
    rec = k.empty((int(L.tdr_map_rec_floats_total(ncls, rows, cols)),))
    ws = k.empty((int(L.tdr_map_ingest_workspace_bytes(ncls, rows, cols)),), torch.uint8)
    maps_d = k.empty((ncls * rows * cols,))
    mask_d = k.empty((rows * cols,), torch.uint8)
    img_t = torch.from_numpy(img.reshape(-1))
    t_up = wall(lambda: img_d.copy_(img_t), reps)
    t_ing = events(lambda: check(L.tdr_k_map_from_labels(_ptr(img_d), size, size, _ptr(lut_d), 256, ncls, C.c_float(res),
                                                         _ptr(rec), _ptr(ws), k.stream())), reps)
    host = {}

    def copies():
        check(L.tdr_k_unpack_map(_ptr(rec), ncls, rows, cols, _ptr(maps_d), _ptr(mask_d), k.stream()))
        host["maps"] = maps_d.cpu().numpy()
        host["mask"] = mask_d.cpu().numpy()
    t_copy = wall(copies, reps)
    dm = DeviceMap(rec, ncls, rows, cols, res)
    t_cmp = wall(lambda: dm.compact(k), reps)
    maps_h = host["maps"]
    t_road = wall(lambda: bool((maps_h[rows * cols:2 * rows * cols] != 0).any()), reps)
    del maps_d, mask_d, ws, dm, img_pin
    print(f"full path by stage: upload {t_up:.2f} ms (wall, pageable), ingest {t_ing:.2f} ms (events), "
          f"host copies {t_copy:.2f} ms (wall: unpack + {4 * ncls * rows * cols / 2**20:.0f} + {rows * cols / 2**20:.0f} MiB "
          f"to the host), compaction {t_cmp:.2f} ms (wall), road scan {t_road:.2f} ms (wall, NumPy)")

    # ---- the handle: full call, incremental calls, patch ----
    m = vp()
    check(L.tdr_map_create(C.byref(m)))
    check(L.tdr_map_sample_pts_polar(m, 100, 25, C.c_float(2 * np.pi / 100)))

    def set_full(im):
        check(L.tdr_map_set_labels(m, im.ctypes.data_as(vp), size, size, lut.ctypes.data_as(vp), 256, ncls, C.c_float(res),
                                   0, 0))
    set_full(img)
    t_full = wall(lambda: set_full(img), reps)
    print(f"tdr_map_set_labels (full update): {t_full:.2f} ms (wall)")
    ch = C.c_int64(0)
    cy, cx = size // 3, size // 4
    for side in (1, 64, 256, 1024):
        new = img.copy()
        new[cy:cy + side, cx:cx + side] = (new[cy:cy + side, cx:cx + side] + 1) % ncls
        ts = []
        for _ in range(reps):
            set_full(img)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check(L.tdr_map_update_labels_incremental(m, new.ctypes.data_as(vp), size, size, lut.ctypes.data_as(vp), 256,
                                                      ncls, C.c_float(res), 0, 0, C.byref(ch)))
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts_p = []
        patch = np.ascontiguousarray(new[cy:cy + side, cx:cx + side])
        for _ in range(reps):
            set_full(img)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check(L.tdr_map_patch_labels(m, patch.ctypes.data_as(vp), cy, cx, side, side, 0, 0, C.byref(ch)))
            torch.cuda.synchronize()
            ts_p.append((time.perf_counter() - t0) * 1e3)
        print(f"change {side} x {side} = {side * side} cells ({ch.value} changed): incremental {np.median(ts):.2f} ms, "
              f"patch {np.median(ts_p):.2f} ms (wall)")
    # the kernel-level launcher alone (device time between events, including its two host round trips)
    km = k.make_map_from_labels(img, lut, ncls, res, keep_ingest=True)
    for side in (1, 64, 256, 1024):
        new = img.copy()
        new[cy:cy + side, cx:cx + side] = (new[cy:cy + side, cx:cx + side] + 1) % ncls
        ts = []
        for _ in range(reps):
            k.update_map_from_labels(km, img)
            ts.append(events(lambda: k.update_map_from_labels(km, new), 1))
        print(f"tdr_k_map_update_labels, {side} x {side}: {np.median(ts):.2f} ms (events; upload, detect, tiles, passes, "
              f"compact refresh)")
    L.tdr_map_destroy(m)


if __name__ == "__main__":
    main()
