"""Batched filter step (tdr_batch_step) against the same filters stepped one after the other: K filters x N particles on
one map, nb x nr polar bins.  Prints one JSON line per K: ms per step of both, and how many filters the batch stepped on
its batched path / through their standalone calls.  Launch counts: run it under
`rocprofv3 --kernel-trace --stats -- python tools/time_batch.py ...`.

    python tools/time_batch.py --ks 1 8 64 --n 20000 --map-size 4000 --steps 20 --warmup 5

--first-update: the wall clock of the FIRST step_batch of K cold-started filters (no particle has a heading: every filter
runs the 40-rotation search) with the init search outside the batch (tdr_config_tuning("batch_init_search") = 0: each
filter's standalone calls) and inside it (1); the filters are stepped once beforehand and set back to their cold states, so
every buffer exists.  --gated: the steady state of a force_on_map fleet (a tenth of the particles start off the map; such a
filter may hold a particle without a heading for ever), switch off against switch on.  --switch 0|1: one of the two only
(launch-count traces).  One JSON line per K: the median, fastest and slowest of --reps runs in ms."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--nb", type=int, default=100)
    ap.add_argument("--nr", type=int, default=25)
    ap.add_argument("--map-size", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("standalone", "batched"), default=None, help="time one mode (launch-count traces)")
    ap.add_argument("--first-update", action="store_true", help="first step of K cold-started filters, switch off / on")
    ap.add_argument("--gated", action="store_true", help="steady state of a force_on_map fleet, switch off / on")
    ap.add_argument("--switch", type=int, choices=(0, 1), default=None, help="with --first-update / --gated: one setting only")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from top_down_renderer_amd import _lib, batch, synth
    cfg = synth.Config("time_batch", 20000, 6, args.nb, args.nr, args.map_size, args.n, seed=4)
    sc = synth.make_scene(cfg)
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, float(cfg.ang_res))
    fp = _lib.FilterParamsC()
    fp.pos_cov, fp.theta_cov, fp.regularization = 0.3, np.pi / 100, 0.15
    fp.init_pos_px_x = fp.init_pos_px_y = fp.init_pos_px_cov = -1
    fp.init_pos_m_x = fp.init_pos_m_y = float("inf")
    fp.init_pos_deg_theta, fp.init_pos_deg_cov = float("inf"), 10
    fp.fixed_scale, fp.scale_log_min, fp.scale_log_max, fp.num_classes = 1.0, -0.1, 1.0, 6
    for i in range(6):
        fp.class_weights[i] = 1.0
    rng = np.random.default_rng(1)
    scan = (rng.integers(0, 4, (6, cfg.nb, cfg.nr)) * (rng.random((6, cfg.nb, cfg.nr)) < 0.2)).astype(np.float32)
    if args.first_update or args.gated:
        return init_modes(args, torch, batch, synth, cfg, sc, m, fp, scan)
    for k in args.ks:
        runs = {}
        for mode in ((args.only,) if args.only else ("standalone", "batched")):
            fs = []
            for i in range(k):
                f = batch.FilterHandle(m, args.n, fp, seed=100 + i)
                f.configure(1, 0)   # like for like: the batch does not compute the locality order either
                f.set_states(synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(i), n=args.n))
                fs.append(f)
            priors = [(1.0, 0.1, 0.01)] * k

            def step():
                if mode == "batched":
                    return batch.step_batch(fs, [scan] * k, cfg.res, priors)
                for f in fs:
                    f.propagate(*priors[0])
                    f.update(scan, cfg.res)
                return (0, k)
            stats = None
            for _ in range(args.warmup):
                stats = step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                stats = step()
            torch.cuda.synchronize()
            runs[mode] = ((time.perf_counter() - t0) * 1e3 / args.steps, stats)
            del fs
        if args.only:
            print(json.dumps({"k": k, "mode": args.only, "ms": round(runs[args.only][0], 4), "steps": args.steps}), flush=True)
            continue
        print(json.dumps({"k": k, "n": args.n, "bins": [cfg.nb, cfg.nr], "map": args.map_size,
                          "standalone_ms": round(runs["standalone"][0], 4), "batched_ms": round(runs["batched"][0], 4),
                          "speedup": round(runs["standalone"][0] / runs["batched"][0], 3),
                          "batched_filters": runs["batched"][1][0], "standalone_filters": runs["batched"][1][1]}),
              flush=True)


def init_modes(args, torch, batch, synth, cfg, sc, m, fp, scan):
    switches = (0, 1) if args.switch is None else (args.switch,)
    try:
        for k in args.ks:
            out = {"k": k, "n": args.n, "bins": [cfg.nb, cfg.nr], "map": args.map_size,
                   "mode": "first_update" if args.first_update else "gated"}
            for sw in switches:
                batch.set_init_search_in_batch(bool(sw))
                if args.gated:
                    fp.force_on_map = 1
                cold = []
                for i in range(k):
                    st = synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(i), n=args.n)
                    st["have_init"] = 0
                    if args.gated:
                        st["init_x_px"][::10] = -50.0
                    cold.append(st)
                fs = [batch.FilterHandle(m, args.n, fp, seed=100 + i) for i in range(k)]
                for f in fs:
                    f.configure(1, 0)
                priors = [(1.0, 0.1, 0.01)] * k
                ms, stats = [], None
                if args.first_update:
                    for rep in range(args.reps + 1):   # (rep 0: the warm-up that allocates)
                        for f, st in zip(fs, cold):
                            f.set_states(st)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        stats = batch.step_batch(fs, [scan] * k, cfg.res, priors)
                        torch.cuda.synchronize()
                        if rep:
                            ms.append((time.perf_counter() - t0) * 1e3)
                else:
                    for f, st in zip(fs, cold):
                        f.set_states(st)
                    for _ in range(args.warmup):
                        batch.step_batch(fs, [scan] * k, cfg.res, priors)
                    for rep in range(args.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            stats = batch.step_batch(fs, [scan] * k, cfg.res, priors)
                        torch.cuda.synchronize()
                        ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
                ms.sort()
                out[f"switch{sw}_ms"] = [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]
                out[f"switch{sw}_filters"] = list(stats)
                del fs
            if len(switches) == 2:
                out["speedup"] = round(out["switch0_ms"][0] / out["switch1_ms"][0], 3)
            print(json.dumps(out), flush=True)
    finally:
        batch.set_init_search_in_batch(False)


if __name__ == "__main__":
    main()
