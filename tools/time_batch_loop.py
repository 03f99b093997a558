"""Batched node loop (top_down_renderer_amd.batch.LoopBatch: tdr_batch_render_polar + tdr_batch_step + tdr_batch_pose +
publishPoseEst) against K standalone loops (per robot: render_polar, propagate, update, publishPoseEst over the filter's
own calls): K robots x N particles on one map, nb x nr polar bins, one cloud of P points per robot.  Wall clock per step
over --steps steps after --warmup, with a device synchronise at the end of the window.  --gmm-every g runs both modes with
the adaptive particle count (CoreConfig.gmm_every: a device mixture fit every g-th step; the counts reached are reported).
Prints one JSON line per K.  Launch
counts: run one mode under `rocprofv3 --kernel-trace --stats -- python tools/time_batch_loop.py ... --only <mode>`.

    python tools/time_batch_loop.py --ks 1 8 64 --n 20000 --points 100000 --map-size 4000 --steps 200 --warmup 10"""
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
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--map-size", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gmm-every", type=int, default=0,
                    help="CoreConfig.gmm_every: refit the mixture on the device every g-th step and adapt the particle count")
    ap.add_argument("--only", choices=("standalone", "batched"), default=None, help="time one mode (launch-count traces)")
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from top_down_renderer_amd import batch, synth
    from top_down_renderer_amd.particle_filter import FilterParams
    from top_down_renderer_amd.top_down_render_core import CoreConfig, TopDownRenderCore
    cfg = synth.Config("time_batch_loop", 20000, 6, args.nb, args.nr, args.map_size, args.n, seed=4)
    sc = synth.make_scene(cfg)
    ncls = sc.class_maps.shape[0]
    ang_res = float(np.float32(2 * np.pi / cfg.nb))
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(cfg.nb, cfg.nr, ang_res)
    fp = FilterParams(fixed_scale=1.0).to_c(ncls)
    ccfg = CoreConfig(theta_bins=cfg.nb, range_bins=cfg.nr, gmm_every=args.gmm_every)
    prior = (1.0, 0.1, 0.01)
    for k in args.ks:
        rng = np.random.default_rng(k)
        clouds = []
        for i in range(k):   # each robot's own cloud: the scene's points resampled and jittered to --points
            sel = rng.integers(0, len(sc.pts), args.points)
            p = sc.pts[sel].copy()
            p[:, :2] += rng.normal(0, 0.05, (args.points, 2)).astype(np.float32)
            clouds.append((np.ascontiguousarray(p, np.float32), 4, 3))
        runs = {}
        for mode in ((args.only,) if args.only else ("standalone", "batched")):
            fs, rs, cores = [], [], []
            for i in range(k):
                f = batch.FilterHandle(m, args.n, fp, seed=100 + i)
                f.set_states(synth.make_particles(cfg, sc.lab, sc.pose, np.random.default_rng(i), n=args.n))
                fs.append(f)
                rs.append(batch.Renderer(sc.lut))
                cores.append(TopDownRenderCore(ccfg))
            loop = batch.LoopBatch(fs, rs, ccfg, ang_res, ncls, cfg.nb, cfg.nr)

            def step():
                if mode == "batched":
                    loop.take_step(clouds, [prior] * k)
                    return loop.stats
                for f, r, c, (pts, stride, ioff) in zip(fs, rs, cores, clouds):
                    c.last_res_ = c.current_range_scale_
                    res = float(c.current_range_scale_)
                    r.render_polar(pts, stride, ioff, res, ang_res, ncls, cfg.nb, cfg.nr)
                    f.propagate(*prior)
                    f.update(r, res, n_target=f.adaptive_count() if args.gmm_every > 0 else -1)
                    c.filter_ = batch.HandleView(f)
                    c.publishPoseEst()
                    c.filter_ = None
                    if c.countStepAndGmmDue():
                        f.compute_gmm(device=True)
                return (0, k)
            stats = None
            for _ in range(args.warmup):
                stats = step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                stats = step()
            torch.cuda.synchronize()
            counts = sorted(f.num_particles() for f in fs)
            runs[mode] = ((time.perf_counter() - t0) * 1e3 / args.steps, stats, [counts[0], counts[len(counts) // 2], counts[-1]])
            del loop, fs, rs
        if args.only:
            print(json.dumps({"k": k, "mode": args.only, "ms": round(runs[args.only][0], 4), "steps": args.steps}), flush=True)
            continue
        print(json.dumps({"k": k, "n": args.n, "bins": [cfg.nb, cfg.nr], "points": args.points, "map": args.map_size,
                          "steps": args.steps, "standalone_ms": round(runs["standalone"][0], 4),
                          "batched_ms": round(runs["batched"][0], 4),
                          "speedup": round(runs["standalone"][0] / runs["batched"][0], 3),
                          "batched_filters": runs["batched"][1][0], "standalone_filters": runs["batched"][1][1],
                          "gmm_every": args.gmm_every, "particles_min_median_max": runs["batched"][2]}),
              flush=True)


if __name__ == "__main__":
    main()
