"""Batched filter step (tdr_batch_step) against the same filters stepped one after the other: K filters x N particles on
one map, nb x nr polar bins.  Prints one JSON line per K: ms per step of both, and how many filters the batch stepped on
its batched path / through their standalone calls.  Launch counts: run it under
`rocprofv3 --kernel-trace --stats -- python tools/time_batch.py ...`.

    python tools/time_batch.py --ks 1 8 64 --n 20000 --map-size 4000 --steps 20 --warmup 5"""
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


if __name__ == "__main__":
    main()
