"""The recovery injection (csrc/tdr_recover.hip, csrc/tdr_host_recover.cpp) timed on one MI355X, one process, medians of --reps:

  road_list   HIP events around tdr_k_map_road_cells (count, running sum, write) on a --map-size x --map-size map of 6
              classes, and the host clock around the first tdr_map_road_cells of a handle on that map (allocation, the three
              launches, the 8-byte read-back);
  inject      HIP events around tdr_k_inject and the host clock around tdr_filter_inject, with the count read back and
              without (then with a device wait of the tool's own), at --particles particles for p = 0.05 and p = 1, both
              heading modes;
  update      the host clock around tdr_filter_update of that filter on a 256 x 256 polar scan: a plain update (every
              particle has a heading), and the update after a heading_mode 0 injection at p = 0.05 and p = 1 (the 40-rotation
              search runs for the injected particles).  The states are put back before every repetition.

The map's distance values are two-valued (0 on the class, 3 elsewhere; unknown cells 0): no timing here depends on them but
through the share of road cells, which is printed.  Writes one JSON line per cell, times in ms, to --out and to stdout.

    python tools/time_recovery.py --out profiles/time_recovery_v1.txt"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np


def summary(ms):
    return {"min": round(min(ms), 4), "median": round(statistics.median(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--map-size", type=int, default=4000)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "time_recovery needs a HIP device"
    torch.cuda.set_device(0)
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib, batch, synth
    from top_down_renderer_amd.kernels import HipKernels
    k, L = HipKernels(), _lib.load()
    sync = torch.cuda.synchronize
    out_f = open(args.out, "w") if args.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    def wall(fn, reset=lambda: None):
        ms = []
        for rep in range(args.warmup + args.reps):
            reset()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return summary(ms)

    def events(fn, reset=lambda: None):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for rep in range(args.warmup + args.reps):
            reset()
            sync()
            ev[0].record()
            fn()
            ev[1].record()
            sync()
            if rep >= args.warmup:
                ms.append(ev[0].elapsed_time(ev[1]))
        return summary(ms)

    cfg = synth.Config("time_recovery", 100000, 6, 256, 256, args.map_size, args.particles, seed=1235)
    rng = np.random.default_rng(cfg.seed)
    lab = synth.make_label_image(cfg.map_size, cfg.ncls, rng)
    maps = np.full((cfg.ncls, cfg.map_size, cfg.map_size), 3.0, np.float32)
    for c in range(cfg.ncls):
        maps[c][(lab == c) | (lab < 0)] = 0.0
    mask = (lab < 0).astype(np.uint8)
    pose = synth.pick_true_pose(lab, rng, 300)
    pts = synth.make_scan(cfg, lab, pose, rng)

    # ---- the road list
    dm = k.make_map(maps, mask, 1.0)
    cells = k.empty((dm.rows * dm.cols,), torch.int32)
    ws = k.empty((int(L.tdr_map_road_workspace_bytes(dm.rows, dm.cols)),), torch.uint8)
    count = k.zeros((1,), torch.int64)
    row = {"road_list": [dm.rows, dm.cols, cfg.ncls],
           "launch": events(lambda: _lib.check(L.tdr_k_map_road_cells(C.byref(dm.desc), cells.data_ptr(), count.data_ptr(),
                                                                      ws.data_ptr(), k.stream())))}
    row["road_cells"] = int(count.item())
    row["road_share"] = round(row["road_cells"] / (dm.rows * dm.cols), 4)
    m = batch.MapHandle(maps, mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    ptr, n_road = C.c_void_p(), C.c_int64(0)
    sync()
    t0 = time.perf_counter()
    _lib.check(L.tdr_map_road_cells(m.h, C.byref(ptr), C.byref(n_road)))
    row["handle_first_call"] = round((time.perf_counter() - t0) * 1e3, 4)
    t0 = time.perf_counter()
    _lib.check(L.tdr_map_road_cells(m.h, C.byref(ptr), C.byref(n_road)))
    row["handle_cached_call"] = round((time.perf_counter() - t0) * 1e3, 4)
    assert n_road.value == row["road_cells"]
    emit(row)

    # ---- the injection
    n = args.particles
    st = synth.make_particles(cfg, lab, pose, rng, n=n)
    dev0 = k.zeros((7, n))
    k.states_to_device(st, dev0, n)
    dev = dev0.clone()
    road = cells[: row["road_cells"]]
    f = batch.FilterHandle(m, n, pkg.FilterParams(fixed_scale=1.0), seed=3)
    r = batch.Renderer(synth.make_lut(cfg.ncls))
    r.render_polar(pts, 4, 3, cfg.res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    for p in (0.05, 1.0):
        th = k.inject_threshold(p)
        for mode in (0, 1):
            cnt = k.zeros((1,), torch.int64)
            row = {"inject": n, "p": p, "heading_mode": mode,
                   "launch": events(lambda: _lib.check(L.tdr_k_inject(dev.data_ptr(), n, n, 0, C.byref(dm.desc), road.data_ptr(),
                                                                      road.numel(), 7, 1, th, mode, cnt.data_ptr(), k.stream())),
                                    lambda: (dev.copy_(dev0), cnt.zero_())),
                   "call_counted": wall(lambda: f.inject(p, mode, 7), lambda: f.set_states(st)),
                   "call_no_readback": wall(lambda: f.inject(p, mode, 7, count=False), lambda: f.set_states(st))}
            f.set_states(st)
            row["injected"] = f.inject(p, mode, 7)
            emit(row)

    # ---- the next update
    def prepare(p):
        f.set_states(st)
        f.propagate(0.2, 0.0, 0.0)
        if p > 0:
            f.inject(p, 0, 7, count=False)

    for p in (0.0, 0.05, 1.0):
        emit({"update_after_inject": n, "p": p, "heading_mode": 0, "scan": [cfg.nb, cfg.nr],
              "update": wall(lambda: f.update(r, cfg.res), lambda: prepare(p))})
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
