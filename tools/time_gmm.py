"""The mixture fit behind the adaptive particle count, host against device (csrc/tdr_gmm.cpp, csrc/tdr_gmm.hip), timed on one
MI355X, one process, medians of --reps:

  call        host clock around tdr_filter_compute_gmm and tdr_filter_compute_gmm_device of twin handles (the cluster count
              is put back before every call, so every repetition makes the same fits);
  kernels     HIP events around tdr_k_gmm_samples, the candidate fits' launch (tdr_k_gmm_fit_jobs) and tdr_k_gmm_pick on
              torch buffers;
  batch       host clock around one tdr_batch_compute_gmm of K filters against K tdr_filter_compute_gmm calls;

per particle set: `two`, `three` and `wide` of tests/test_gmm_device.py and eight clusters of sigma = 40 px.  Prints one JSON
line per cell, times in ms.

    python tools/time_gmm.py --batch 1 8 64"""
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


def clusters(seed, centres, sig, n_each, sig_theta):
    rng = np.random.default_rng(seed)
    xs = []
    for (cx, cy, th), s in zip(centres, sig):
        xy = rng.normal([cx, cy], s, (n_each, 2))
        xs.append(np.column_stack([xy, rng.normal(th, sig_theta, n_each)]))
    x = np.concatenate(xs)
    return x[rng.permutation(len(x))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--particles", type=int, default=20000)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "time_gmm needs a HIP device"
    torch.cuda.set_device(0)
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib, batch, synth
    from top_down_renderer_amd.kernels import HipKernels
    k, L = HipKernels(), _lib.load()
    sync = torch.cuda.synchronize
    sc = synth.make_scene("c1", n_particles=64)          # any map: the fit reads particle states only
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(sc.cfg.nb, sc.cfg.nr, float(sc.cfg.ang_res))
    fp = pkg.FilterParams(fixed_scale=1.0).to_c(sc.class_maps.shape[0])
    rng8 = np.random.default_rng(4)
    sets = {"two": (clusters(6, [(100, 200, 0.3), (400, 250, -2.0)], [10, 10], 400, 0.001), 2),
            "three": (clusters(5, [(100, 200, 0.3), (400, 250, -2.0), (250, 600, 1.5)], [8, 15, 5], 300, 0.001), 3),
            "wide": (clusters(9, [(500, 500, 0)], [150], 1000, 1.5), 1),
            "eight": (clusters(10, [(rng8.uniform(100, 900), rng8.uniform(100, 900), rng8.uniform(-3, 3)) for _ in range(8)],
                               [40] * 8, 125, 0.05), 8)}

    def states(xyt, n):
        st = np.zeros(n, batch.STATE_DTYPE)
        src = np.arange(n) * len(xyt) // n
        st["init_x_px"], st["init_y_px"], st["theta"] = xyt[src, 0], xyt[src, 1], xyt[src, 2]
        st["scale"], st["have_init"] = 1.0, 1
        return st

    def handle(xyt, start, n=None):
        f = batch.FilterHandle(m, n or args.particles, fp, seed=3)
        f.set_states(states(xyt, n or args.particles))
        f.set_num_gaussians(start)
        return f

    def wall(fn, reset):
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

    for name, (xyt, start) in sets.items():
        fh, fd = handle(xyt, start), handle(xyt, start)
        row = {"set": name, "particles": args.particles, "start": start,
               "host_call": wall(lambda: fh.compute_gmm(device=False), lambda: fh.set_num_gaussians(start)),
               "device_call": wall(lambda: fd.compute_gmm(device=True), lambda: fd.set_num_gaussians(start)),
               "chosen": [fh.num_gaussians(), fd.num_gaussians()]}
        # the launches on torch buffers
        n, num = args.particles, min(1000, args.particles)
        dev = k.zeros((7, n))
        k.states_to_device(states(xyt, n), dev, n)
        ml3 = k.sample_ml_states(dev, n, num)
        cand = k.gmm_candidates(start, n, num)
        x = k.gmm_samples(ml3, num)
        jobs, pick, keep = [], _lib.GmmPickJobC(), []
        pick.k = cand[0]
        for j, kc in enumerate(cand):
            if kc:
                out, ws = k.zeros((21 * kc + 2,), torch.float64), k.empty((num * kc,), torch.float64)
                keep += [out, ws]
                jobs.append(_lib.GmmJobC(x.data_ptr(), num, kc, 100, 0, out.data_ptr(), ws.data_ptr()))
                pick.cand[j] = out.data_ptr()
        rec = k.zeros((_lib.GMM_RECORD_DOUBLES,), torch.float64)
        pick.record = rec.data_ptr()
        jd = k.to_device(np.frombuffer(bytes((_lib.GmmJobC * len(jobs))(*jobs)), np.uint8))
        pd = k.to_device(np.frombuffer(bytes(pick), np.uint8))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        times = {"samples": [], "fits": [], "pick": []}
        for rep in range(args.warmup + args.reps):
            ev[0].record()
            _lib.check(L.tdr_k_gmm_samples(ml3.data_ptr(), num, x.data_ptr(), k.stream()))
            ev[1].record()
            _lib.check(L.tdr_k_gmm_fit_jobs(jd.data_ptr(), len(jobs), k.stream()))
            ev[2].record()
            _lib.check(L.tdr_k_gmm_pick(pd.data_ptr(), 1, k.stream()))
            ev[3].record()
            sync()
            if rep >= args.warmup:
                for i, key in enumerate(times):
                    times[key].append(ev[i].elapsed_time(ev[i + 1]))
        o = [t.cpu().numpy() for t in keep[::2]]
        row.update(candidates=cand, e_steps=[int(a[-1]) for a in o], launches={key: summary(v) for key, v in times.items()})
        print(json.dumps(row), flush=True)

    names = list(sets)
    for K in args.batch:
        fb = [handle(*sets[names[i % len(names)]]) for i in range(K)]
        fh = [handle(*sets[names[i % len(names)]]) for i in range(K)]
        starts = [sets[names[i % len(names)]][1] for i in range(K)]

        def reset(fs):
            for f, s in zip(fs, starts):
                f.set_num_gaussians(s)

        def host_calls():
            for f in fh:
                f.compute_gmm(device=False)

        print(json.dumps({"batch": K, "particles": args.particles,
                          "batch_call": wall(lambda: batch.compute_gmm_batch(fb), lambda: reset(fb)),
                          "host_calls": wall(host_calls, lambda: reset(fh))}), flush=True)


if __name__ == "__main__":
    main()
