"""The pose-grid search (csrc/tdr_grid.hip, csrc/tdr_host_grid.cpp) timed on one MI355X, one process, medians of --reps, at the
shape of tools/time_recovery_sensor.py (100 000 particles, a 4000 x 4000 map of 6 classes, a 256 x 256 polar scan, fixed
scale).  Lattices: road cells only over the whole map at step 16, 8 and 4; no heading (the 40-rotation search), and 1 and 8
fixed headings.

  list        HIP events around tdr_k_grid_list (count, running sum, write);
  peaks       HIP events around tdr_k_grid_peaks on the call's W plane (R = 2, K = 8): the tile pass, the radix sort of the
              key plane, the emit;
  call        the host clock around tdr_filter_grid_search with every output read back (W, T, 8 peaks), and with none
              (`call_no_readback`: the count of peaks alone): the difference is the read-back of the two planes;
  weights     the host clock around tdr_filter_compute_weights of a second filter that holds the same lattice states through
              set_states: the scoring launches without the list, the candidates, the reduction and the peaks (n_total is
              that filter's own count there, so the figures are comparable, not the same launches).
Writes one JSON line per cell, times in ms, to --out and to stdout.

    python tools/time_grid_search.py --out profiles/time_grid_search_v1.txt"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--map-size", type=int, default=4000)
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--steps", type=int, nargs="*", default=[16, 8, 4])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "time_grid_search needs a HIP device"
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

    def wall(fn):
        ms = []
        for rep in range(args.warmup + args.reps):
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
    f.set_states(st)
    r = batch.Renderer(synth.make_lut(cfg.ncls))
    r.render_polar(pts, 4, 3, cfg.res, float(cfg.ang_res), cfg.ncls, cfg.nb, cfg.nr)
    dm = k.make_map(maps, mask, 1.0)
    road = m.road_cells().astype(np.int64)
    rr, rc = road // cfg.map_size, road % cfg.map_size
    res_c = C.c_float(cfg.res)

    for step in args.steps:
        off = step // 2
        npts = (cfg.map_size - off + step - 1) // step
        on = ((rr - off) % step == 0) & ((rc - off) % step == 0)
        for mode, H in ((0, 1), (1, 1), (1, 8)):
            spec = _lib.grid_spec(off, off, step, npts, npts, 1, mode, H, -np.pi, 2 * np.pi / H, 1.0)
            G = npts * npts
            # the list launch alone
            lst = k.empty((G,), torch.int32)
            ws = k.empty((max(8, int(L.tdr_grid_list_workspace_bytes(npts, npts))),), torch.uint8)
            count = k.zeros((1,), torch.int64)
            row = {"grid_search": n, "step": step, "lattice": [npts, npts], "heading_mode": mode, "n_headings": H,
                   "scan": [cfg.nb, cfg.nr], "inject_cand_chunk": k.tuning("inject_cand_chunk"),
                   "list": events(lambda: _lib.check(L.tdr_k_grid_list(C.byref(dm.desc), C.byref(spec), lst.data_ptr(), count.data_ptr(),
                                                                       ws.data_ptr(), 0, k.stream())))}
            row["listed"] = int(count.item())
            assert row["listed"] == int(on.sum())
            row["candidates"] = row["listed"] * H
            # the call
            row["call"] = wall(lambda: f.grid_search(r, cfg.res, spec, 2, 8))
            got = f.grid_search(r, cfg.res, spec, 2, 8)
            n_peaks = C.c_int64(0)
            row["call_no_readback"] = wall(lambda: _lib.check(L.tdr_filter_grid_search(f.h, None, r.h, res_c, C.byref(spec), None, None, None,
                                                                                       2, 8, None, C.byref(n_peaks), None)))
            assert n_peaks.value == got.n_peaks
            row["n_peaks"] = got.n_peaks
            row["us_per_candidate"] = round(row["call"]["median"] * 1e3 / max(row["candidates"], 1), 4)
            # the peak search alone, on the call's planes
            gw, gt = k.to_device(got.w.ravel()), k.to_device(got.theta.ravel())
            pws = k.empty((max(8, int(L.tdr_grid_peaks_workspace_bytes(npts, npts))),), torch.uint8)
            pk = k.zeros((8, 4), torch.int32)
            row["peaks"] = events(lambda: _lib.check(L.tdr_k_grid_peaks(C.byref(dm.desc), C.byref(spec), gw.data_ptr(), gt.data_ptr(), 2, 8,
                                                                        pk.data_ptr(), count.data_ptr(), pws.data_ptr(), k.stream())))
            # the same states scored by a filter that holds them
            cand = np.zeros((row["listed"], H), batch.STATE_DTYPE)
            cand["init_x_px"] = (rc[on].astype(np.float32) + np.float32(0.5))[:, None]
            cand["init_y_px"] = (rr[on].astype(np.float32) + np.float32(0.5))[:, None]
            cand["scale"] = 1.0
            if mode == 1:
                cand["theta"] = (np.float32(spec.theta0) + np.arange(H).astype(np.float32) * np.float32(spec.dtheta))[None, :]
                cand["have_init"] = 1
            g = batch.FilterHandle(m, cand.size, pkg.FilterParams(fixed_scale=1.0), seed=4)
            flat = np.ascontiguousarray(cand.reshape(-1))

            def weights():
                g.set_states(flat)
                sync()
                t0 = time.perf_counter()
                g.compute_weights(r, cfg.res)
                sync()
                return (time.perf_counter() - t0) * 1e3
            ms = [weights() for _ in range(args.warmup + args.reps)][args.warmup:]
            row["weights_of_a_filter_holding_the_states"] = summary(ms)
            del g
            emit(row)
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
