"""The KLD-sampling count (csrc/tdr_kld.hip, csrc/tdr_host_kld.cpp) timed on one MI355X, one process, medians of --reps:

  launch      HIP events around tdr_k_kld_count on torch buffers: the table's fill, the clearing of the two output words and
              the kernel (`fill` alone: the same events around a fill of the table's size);
  call        host clock around tdr_filter_kld_count (the launch plus its 16-byte read-back and wait);
  gmm_call    host clock around tdr_filter_compute_gmm_device of a twin handle at the same particle count — the rule the
              count can stand in for (the cluster count is put back before every call);
  batch       host clock around one tdr_batch_kld_count of K filters against K tdr_filter_kld_count calls;

per particle set: `cluster` (a converged cloud, a handful of bins), `c5` (config 5's 8 clusters x 40 headings) and `uniform`
(k close to n).  Prints one JSON line per cell, times in ms.

    python tools/time_kld.py --particles 20000 100000 2000000 --batch 16 64"""
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


def make_states(kind, n, dtype, seed=1):
    rng = np.random.default_rng(seed)
    st = np.zeros(n, dtype)
    if kind == "cluster":
        st["init_x_px"], st["init_y_px"] = rng.normal(2000, 1.5, n), rng.normal(1800, 1.5, n)
        st["theta"] = rng.normal(0.4, 0.02, n)
    elif kind == "c5":
        c = rng.uniform(500, 3500, (8, 2))
        g = rng.integers(0, 8, n)
        st["init_x_px"], st["init_y_px"] = rng.normal(c[g, 0], 40), rng.normal(c[g, 1], 40)
        st["theta"] = (rng.integers(0, 40, n) * (2 * np.pi / 40) - np.pi).astype(np.float32)
    else:
        st["init_x_px"], st["init_y_px"] = rng.uniform(0, 4000, n), rng.uniform(0, 4000, n)
        st["theta"] = rng.uniform(-np.pi, np.pi, n)
    st["scale"], st["have_init"] = 1.0, 1
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--particles", type=int, nargs="*", default=[20000, 100000, 2000000])
    ap.add_argument("--batch", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--batch-particles", type=int, default=20000)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "time_kld needs a HIP device"
    torch.cuda.set_device(0)
    import top_down_renderer_amd as pkg
    from top_down_renderer_amd import _lib, batch, synth
    from top_down_renderer_amd.kernels import HipKernels
    k, L = HipKernels(), _lib.load()
    sync = torch.cuda.synchronize
    sc = synth.make_scene("c1", n_particles=64)          # any map: the count reads particle states only
    m = batch.MapHandle(sc.class_maps, sc.class_mask, 1.0)
    m.sample_pts_polar(sc.cfg.nb, sc.cfg.nr, float(sc.cfg.ang_res))
    fp = pkg.FilterParams(fixed_scale=1.0).to_c(sc.class_maps.shape[0])
    params = pkg.KldParams()
    pc = params.to_c()

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

    for n in args.particles:
        for kind in ("cluster", "c5", "uniform"):
            st = make_states(kind, n, batch.STATE_DTYPE)
            dev = k.zeros((7, n))
            k.states_to_device(st, dev, n)
            ws, out = k.kld_workspace(n), k.zeros((2,), torch.int64)
            row = {"set": kind, "particles": n, "table_bytes": ws.numel() * 8,
                   "launch": events(lambda: _lib.check(L.tdr_k_kld_count(dev.data_ptr(), n, n, C.byref(pc), ws.data_ptr(),
                                                                         out.data_ptr(), k.stream()))),
                   "fill": events(lambda: ws.fill_(-1))}
            row["k"], row["skipped"] = out.cpu().tolist()
            f, g = batch.FilterHandle(m, n, fp, seed=3), batch.FilterHandle(m, n, fp, seed=3)
            f.set_states(st)
            g.set_states(st)
            row["call"] = wall(lambda: f.kld_count(params))
            row["target"] = f.kld_count(params)[2]
            row["gmm_call"] = wall(lambda: g.compute_gmm(device=True), lambda: g.set_num_gaussians(1))
            row["gmm_count"] = g.adaptive_count()
            print(json.dumps(row), flush=True)
            del f, g, dev, ws

    names = ("cluster", "c5", "uniform")
    for K in args.batch:
        fs = []
        for i in range(K):
            f = batch.FilterHandle(m, args.batch_particles, fp, seed=3 + i)
            f.set_states(make_states(names[i % 3], args.batch_particles, batch.STATE_DTYPE, seed=i))
            fs.append(f)
        print(json.dumps({"batch": K, "particles": args.batch_particles,
                          "batch_call": wall(lambda: batch.kld_count(fs, params)),
                          "single_calls": wall(lambda: [f.kld_count(params) for f in fs])}), flush=True)


if __name__ == "__main__":
    main()
