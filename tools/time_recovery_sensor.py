"""Sensor resetting (csrc/tdr_recover_sensor.hip, csrc/tdr_host_recover.cpp) timed on one MI355X, one process, medians of
--reps, at the shape of tools/time_recovery.py (its comparison points are profiles/time_recovery_v1.txt):

  list        HIP events around tdr_k_inject_list (count, running sum, write) at --particles slots, p = 0.002 and 0.05;
  call        the host clock around tdr_filter_inject_sensor (the count read back) on a 256 x 256 polar scan, for
              p in {0.002, 0.05}, C in {16, 64} and both heading modes, with the number of candidates scored; next to it
              tdr_filter_inject at the same p and mode;
  update      the host clock around the next tdr_filter_update: plain, after a heading_mode 0 uniform injection (the search
              runs for the injected slots) and after a heading_mode 0 sensor call (the winners have headings).
The states are put back before every repetition.  Writes one JSON line per cell, times in ms, to --out and to stdout.

    python tools/time_recovery_sensor.py --out profiles/time_recovery_sensor_v1.txt"""
import argparse
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--map-size", type=int, default=4000)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "time_recovery_sensor needs a HIP device"
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

    def events(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for rep in range(args.warmup + args.reps):
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
    n = args.particles
    st = synth.make_particles(cfg, lab, pose, rng, n=n)
    m = batch.MapHandle(maps, mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    f = batch.FilterHandle(m, n, pkg.FilterParams(fixed_scale=1.0), seed=3)
    r = batch.Renderer(synth.make_lut(cfg.ncls))
    r.render_polar(pts, 4, 3, cfg.res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    chunk = k.tuning("inject_cand_chunk")

    # ---- the list launch alone
    lst = k.empty((n,), torch.int32)
    ws = k.empty((max(8, int(L.tdr_inject_list_workspace_bytes(n))),), torch.uint8)
    count = k.zeros((1,), torch.int64)
    for p in (0.002, 0.05):
        th = k.inject_threshold(p)
        row = {"list": n, "p": p,
               "launch": events(lambda: _lib.check(L.tdr_k_inject_list(n, 0, 7, 1, th, lst.data_ptr(), count.data_ptr(), ws.data_ptr(), 0,
                                                                       k.stream())))}
        row["listed"] = int(count.item())
        emit(row)

    # ---- the call
    for p in (0.002, 0.05):
        for mode in (0, 1):
            emit({"inject": n, "p": p, "heading_mode": mode,
                  "call_counted": wall(lambda: f.inject(p, mode, 7), lambda: f.set_states(st))})
            for C_ in (16, 64):
                row = {"inject_sensor": n, "p": p, "candidates": C_, "heading_mode": mode, "scan": [cfg.nb, cfg.nr],
                       "inject_cand_chunk": chunk,
                       "call_counted": wall(lambda: f.inject_sensor(r, cfg.res, p, C_, mode, 7), lambda: f.set_states(st))}
                f.set_states(st)
                row["written"] = f.inject_sensor(r, cfg.res, p, C_, mode, 7)
                row["candidates_scored"] = row["written"] * C_
                emit(row)

    # ---- the next update
    def prepare(p, C_):
        f.set_states(st)
        f.propagate(0.2, 0.0, 0.0)
        if p > 0 and C_ == 0:
            f.inject(p, 0, 7, count=False)
        elif p > 0:
            f.inject_sensor(r, cfg.res, p, C_, 0, 7, count=False)

    for p, C_ in ((0.0, 0), (0.05, 0), (0.05, 16), (0.05, 64)):
        emit({"update_after": "nothing" if p == 0 else ("inject" if C_ == 0 else "inject_sensor"), "particles": n, "p": p,
              "candidates": C_, "heading_mode": 0, "scan": [cfg.nb, cfg.nr],
              "update": wall(lambda: f.update(r, cfg.res), lambda: prepare(p, C_))})
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
